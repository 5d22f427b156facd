"""GPU tests of the arithmetic modes across FINITE magnitudes ("Finite dynamic range of the arithmetic modes"): the
rest of the suite feeds every kernel O(1) data, tests/test_hip_nonfinite.py covers NaN and Inf; this module covers what lies
between O(1) and Inf, and between O(1) and zero.

Exact statements (no tolerance).  Exact fp32, Winograd and bf16 arithmetic commute with powers of two: fp32 / bf16 rounding, fmaf,
max, x -> 0.2 x and the Winograd transforms (+, -, * 0.5, * 0.25) all do, as long as nothing overflows or turns subnormal.  So

    K(2^a x, 2^c w, 2^(a+c) b)  ==  ldexp(K(x, w, b), a + c)        bit for bit (np.array_equal),

outputs and - through the helpers of tests/hip_helpers.py - the sentinels between strided frames alike.  A folded BatchNorm is
scaled the homogeneous way: mean and beta with the bias, gamma and var not at all.  Operands are `bounded(emin=-6, emax=1)`.
Why no intermediate leaves the normal range: operands are multiples of 2^-29 below 2^2, BatchNorm-folded weights multiples of
2^-31 below 2^5, so every partial sum of at most 2304 products is a multiple of 2^-60 below 2^19, and |a + c| <= 60 keeps all of
it inside [2^-120, 2^79] (the two-layer fused block: multiples of 2^-91, |a + c0 + c1| <= 30).
A failure here is a bug in that kernel or packer: a hidden fp16 / bf16 intermediate, an absolute epsilon, a packed conversion in
a staging loop, a flush-to-zero compile flag, an epilogue that is not homogeneous.

Split fp16 (VAD_PREC_SPLIT) is held to bounds against float64, derived in `magnitude_ref.split_bound` / `_split_B` below - not
fitted to the kernels -, inside its window, above it (never a finite wrong number) and below it (the documented loss).

Not covered, because none of it commutes with scaling: anything with tanh or sigmoid (the ConvLSTM gates, the tails'
reconstruction), BatchNorm's eps (train-mode BatchNorm, the folding itself), SSIM's C1 / C2, Adam."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import magnitude_ref as M
import test_hip_layers as L
import test_hip_nonfinite as NF
from conftest import load_synthetic, rel_err
from oracle import torch_oracle

pytestmark = pytest.mark.gpu

PAIRS = [(0, 0), (20, 0), (-20, 0), (0, 20), (0, -20), (30, 30), (-30, -30), (40, -40)]
#: (a, c0, c1) of the two-layer fused block (its intermediates carry a + c0, its outputs a + c0 + c1)
TRIPLES = [(0, 0, 0), (20, 0, 0), (-20, 0, 0), (0, 20, 0), (0, -20, 0), (0, 20, -20), (0, 0, 20), (10, 10, 10), (-10, -10, -10), (40, -40, 0)]
EXPONENTS = [0, 20, -20, 40, -40, 60, -60]


@pytest.fixture(autouse=True)
def _fixed_cpu_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(before)


def _data(rng, shape, zeros=0.3, bits=23):
    return M.bounded(rng, shape, -6, 1, zeros, bits)


def _bn(rng, cout):
    """[gamma, beta, mean, var]: gamma and var O(1) and free, beta and mean in the exponent window (they scale with the bias)."""
    return [rng.uniform(0.5, 1.5, cout).astype(np.float32), _data(rng, cout, 0.0), _data(rng, cout, 0.0), rng.uniform(0.25, 1.75, cout).astype(np.float32)]


def _bn_scaled(bn, k):
    return None if bn is None else [bn[0], M.scaled(bn[1], k), M.scaled(bn[2], k), bn[3]]


def _same_bits(tag, got, base, k):
    got, base = np.asarray(got, np.float32), np.asarray(base, np.float32)
    assert got.shape == base.shape and np.isfinite(got).all(), tag
    want = M.scaled(base, k)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{tag}: {len(bad)} of {got.size} elements are not 2^{k} times the unscaled launch's, first at {i}: "
                             f"{got[i]!r} ({float(got[i]).hex()}) vs {want[i]!r} ({float(want[i]).hex()})")


def _live(tag, base):
    """The unscaled result is worth comparing against: finite, not constant, mostly non-zero."""
    base = np.asarray(base, np.float32)
    assert np.isfinite(base).all() and (base != 0).mean() > 0.2 and len(np.unique(base)) > base.size // 8, tag


def _equivariant(tag, forms, run, cases, exponent=sum):
    """run(*case) under every kernel form == ldexp(run(*zeros) under the same form, exponent(case))."""
    for fname, under in forms.items():
        base = under(run, *([0] * len(cases[0])))
        for o in (base if isinstance(base, tuple) else (base,)):
            _live(f"{tag} {fname}", o)
        for case in cases:
            got = under(run, *case)
            for o, (g, b) in enumerate(zip(got if isinstance(got, tuple) else (got,), base if isinstance(base, tuple) else (base,))):
                _same_bits(f"{tag} {fname} {case} out{o}", g, b, exponent(case))


def _forms(l, variants=(), one_cu=True):
    """{label: under(run, *args)}: the default plan, every vad_debug_set_conv_variant value given, the one-CU plan."""
    def ctx(c):
        def under(run, *args):
            with c:
                return run(*args)
        return under
    forms = {"default": lambda run, *args: run(*args)}
    for bits in variants:
        forms[f"variant{bits}"] = ctx(NF._variant(l, bits))
    if one_cu:
        forms["one-cu"] = ctx(NF._plan_cus(l, 1))
    return forms


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _f32(t):
    return t.float().cpu().numpy()


def _bf16(a):
    """bf16 device tensor of bf16-representable fp32 data (by value: checked)."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    t16 = t.to(torch.bfloat16)
    assert torch.equal(t16.float(), t), "the data are not bf16-representable"
    return t16


# =============================================================================== exact statements: scoring layers
@pytest.mark.parametrize("precision", [0, 2], ids=["fp32", "bf16op"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("cin,cout,h,w", [(32, 32, 16, 16), (64, 128, 6, 10)])
def test_conv3x3_scales_exactly(vad, cin, cout, h, w, act, pool, precision):
    """vad_conv3x3, 3 strided frames.  Exact fp32: host-packed weights with a folded BatchNorm under the cost model's plan, the
    persistent-only, gate-split and one-tile forms (1|64, 1|128, 0) and the one-CU plan (a walk over all tiles).  bf16 operands
    (VAD_PREC_BF16): weights from vad_train_pack_conv3x3 (no folding in train mode), default and one-CU plan."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng = L._rng(cin * 1000 + cout + h + 31 + act + 7 * pool)
    x, wt, b = _data(rng, (3, cin, h, w)), _data(rng, (cout, cin, 3, 3), 0.1), _data(rng, cout, 0.0)
    bn = _bn(rng, cout) if precision == 0 else None
    ho, wo = (h // 2, w // 2) if pool else (h, w)

    def run(a, c):
        xs, ws, bs = M.scaled(x, a), M.scaled(wt, c), M.scaled(b, a + c)
        if precision == 0:
            return H.conv3x3(xs, ws, bs, _bn_scaled(bn, a + c), act, pool, fs=H.FS_PAD)
        wd, bd = H.dev(ws), H.dev(bs)
        fwd = _nan(l.vad_pack_conv3x3_floats(cout, cin))
        vad.hip.check(l.vad_train_pack_conv3x3(wd.data_ptr(), cout, cin, fwd.data_ptr(), None, precision, H.stream()))
        xin, out = H._in_frames(xs, H.FS_PAD), H._out_frames(3, (ho, wo, cout), H.FS_PAD)
        vad.hip.check(l.vad_conv3x3(xin.ptr, xin.fs, fwd.data_ptr(), bd.data_ptr(), out.ptr, out.fs, 3, h, w, cin, cout, act, int(pool), precision, H.stream()))
        return H._result(out)

    forms = _forms(l, (1 | 64, 1 | 128, 0)) if precision == 0 else _forms(l)
    _equivariant(f"conv3x3 {cin}->{cout} {h}x{w} act{act} pool{int(pool)} prec{precision}", forms, run, PAIRS)


@pytest.mark.parametrize("cin,cout,h,w,act,pool", [(32, 32, 16, 16, 1, False), (32, 32, 16, 16, 2, True), (64, 64, 5, 9, 0, False), (64, 64, 6, 10, 1, True)])
def test_conv3x3_winograd_scales_exactly(vad, cin, cout, h, w, act, pool):
    """vad_conv3x3_wino: U = G g G^T is rounded once from float64 on the host, the input and output transforms add, subtract and
    halve.  5x9 has partial tiles."""
    import hip_helpers as H
    rng = L._rng(cin * 1000 + cout + h + 32)
    x, wt, b, bn = _data(rng, (3, cin, h, w)), _data(rng, (cout, cin, 3, 3), 0.1), _data(rng, cout, 0.0), _bn(rng, cout)
    run = lambda a, c: H.conv3x3_wino(M.scaled(x, a), M.scaled(wt, c), M.scaled(b, a + c), _bn_scaled(bn, a + c), act, pool, fs=H.FS_PAD)
    _equivariant(f"wino {cin}->{cout} {h}x{w} act{act} pool{int(pool)}", _forms(vad.hip.lib()), run, PAIRS)


@pytest.mark.parametrize("cin,cout,h,w,act", [(64, 32, 3, 5, 2), (128, 64, 4, 4, 0), (32, 32, 9, 13, 1)])
def test_convt2x2_scales_exactly(vad, cin, cout, h, w, act):
    """vad_convt2x2 at VAD_PREC_FP32 with a folded BatchNorm, strided frames, default and one-CU plan."""
    import hip_helpers as H
    rng = L._rng(cin + cout * 7 + h + 33)
    x, wt, b, bn = _data(rng, (3, cin, h, w)), _data(rng, (cin, cout, 2, 2), 0.1), _data(rng, cout, 0.0), _bn(rng, cout)
    run = lambda a, c: H.convt2x2(M.scaled(x, a), M.scaled(wt, c), M.scaled(b, a + c), _bn_scaled(bn, a + c), act, fs=H.FS_PAD)
    _equivariant(f"convt {cin}->{cout} {h}x{w} act{act}", _forms(vad.hip.lib()), run, PAIRS)


@pytest.mark.parametrize("cin,cout", [(64, 32), (64, 96), (128, 128)])
def test_conv1x1_scales_exactly(vad, cin, cout):
    import hip_helpers as H
    rng = L._rng(cin + cout + 34)
    x, wt, b = _data(rng, (3, cin, 5, 7)), _data(rng, (cout, cin, 1, 1), 0.1), _data(rng, cout, 0.0)
    run = lambda a, c: H.conv1x1(M.scaled(x, a), M.scaled(wt, c), M.scaled(b, a + c))
    _equivariant(f"conv1x1 {cin}->{cout}", _forms(vad.hip.lib(), one_cu=False), run, PAIRS)


@pytest.mark.parametrize("npix,cin,cout", [(70, 64, 64), (256, 128, 32), (24, 32, 96)])
def test_conv1x1_bf16_tensors_scales_exactly(vad, npix, cin, cout):
    """vad_conv1x1_p with VAD_PREC_BF16S: bf16 tensors in and out (bf16-representable inputs), the weights rounded to bf16 by
    vad_train_pack_conv1x1_p, fp32 accumulation from an fp32 bias, the result rounded to bf16 - every step commutes with 2^k."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng = L._rng(npix + cin + 35)
    x, wt, b = _data(rng, (npix, cin), bits=7), _data(rng, (cout, cin), 0.1), _data(rng, cout, 0.0)

    def run(a, c):
        xd, wd, bd = _bf16(M.scaled(x, a)), H.dev(M.scaled(wt, c)), H.dev(M.scaled(b, a + c))
        fwd, dgr = _nan(l.vad_pack_conv1x1_floats(cout, cin)), _nan(l.vad_pack_conv1x1_floats(cin, cout))
        vad.hip.check(l.vad_train_pack_conv1x1_p(wd.data_ptr(), cout, cin, fwd.data_ptr(), dgr.data_ptr(), 3, H.stream()))
        out = _nan(npix, cout, dtype=torch.bfloat16)
        vad.hip.check(l.vad_conv1x1_p(xd.data_ptr(), fwd.data_ptr(), bd.data_ptr(), out.data_ptr(), npix, cin, cout, 3, H.stream()))
        torch.cuda.synchronize()
        return _f32(out)

    _equivariant(f"conv1x1_p bf16 {npix}x{cin}->{cout}", _forms(l, one_cu=False), run, PAIRS)


@pytest.mark.parametrize("cout,h,w,act,pool", [(32, 16, 16, 1, False), (32, 16, 16, 1, True), (32, 6, 10, 2, False), (64, 6, 10, 0, True)])
def test_conv3x3_c3_scales_exactly(vad, cout, h, w, act, pool):
    """vad_conv3x3_c3 (the first layer: K = 27 padded to 28 with a zero weight), persistent and one-tile form, one-CU plan; and its
    bf16-output forms vad_conv3x3_c3_bf16 (fp32 arithmetic, the result rounded to bf16) and vad_conv3x3_c3_bf16op (bf16 operands
    too), un-activated and un-pooled as the training step runs them."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng = L._rng(cout + h + w + 36)
    x, wt, b, bn = _data(rng, (3, 3, h, w), 0.1), _data(rng, (cout, 3, 3, 3), 0.0), _data(rng, cout, 0.0), _bn(rng, cout)
    run = lambda a, c: H.conv3x3(M.scaled(x, a), M.scaled(wt, c), M.scaled(b, a + c), _bn_scaled(bn, a + c), act, pool)
    _equivariant(f"conv3x3_c3 ->{cout} {h}x{w} act{act} pool{int(pool)}", _forms(l, (0,)), run, PAIRS)
    if act or pool:
        return
    for name in ("vad_conv3x3_c3_bf16", "vad_conv3x3_c3_bf16op"):
        def run16(a, c):
            wp, bo = H.pack_conv3x3(M.scaled(wt, c), M.scaled(b, a + c), _bn_scaled(bn, a + c))
            xd, out = H.dev(M.scaled(x, a)), _nan(3, h, w, cout, dtype=torch.bfloat16)
            vad.hip.check(getattr(l, name)(xd.data_ptr(), wp.data_ptr(), bo.data_ptr(), out.data_ptr(), 3, h, w, cout, H.stream()))
            torch.cuda.synchronize()
            return _f32(out)
        _equivariant(f"{name} ->{cout} {h}x{w}", _forms(l, one_cu=False), run16, PAIRS)


@pytest.mark.parametrize("h,w", [(16, 16), (22, 18)])
def test_conv3x3_c3_fused_scales_exactly(vad, h, w):
    """The fused enc1 block at VAD_PREC_FP32 (conv 3->32 + LeakyReLU kept in the tile, conv 32->32 + LeakyReLU + pooling): the
    first bias carries 2^(a+c0), the second 2^(a+c0+c1).  Persistent and one-tile form, one-CU plan."""
    import hip_helpers as H
    rng = L._rng(h * 100 + w + 37)
    x = _data(rng, (3, 3, h, w), 0.1)
    w0, b0, bn0 = _data(rng, (32, 3, 3, 3), 0.0), _data(rng, 32, 0.0), _bn(rng, 32)
    w1, b1, bn1 = _data(rng, (32, 32, 3, 3), 0.1), _data(rng, 32, 0.0), _bn(rng, 32)

    def run(a, c0, c1):
        return H.conv3x3_c3_fused(M.scaled(x, a), M.scaled(w0, c0), M.scaled(b0, a + c0), _bn_scaled(bn0, a + c0),
                                  M.scaled(w1, c1), M.scaled(b1, a + c0 + c1), _bn_scaled(bn1, a + c0 + c1))

    _equivariant(f"c3_fused {h}x{w}", _forms(vad.hip.lib(), (0,)), run, TRIPLES)


# ============================================================================== exact statements: training kernels
@pytest.mark.parametrize("shape", __import__("wgrad_identity").SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient_scales_exactly(vad, shape):
    """vad_conv_wgrad at VAD_PREC_FP32, _BF16 and _BF16S (bf16 tensors: bf16-representable operands) in every kernel form that
    vad_conv_wgrad_plan reports for the shape under some setting of the vad_debug_set_wgrad_* switches (tests/wgrad_identity.py:
    per-wave, row-ring, paired-channel and LDS-staged forms, split-K partial slots and their fixed-order reduce).  The operands are
    activations (2^a) and output gradients (2^c).  VAD_PREC_SPLIT: the bounds further down; VAD_PREC_WINO is not a weight-gradient
    mode (the Winograd trainer runs VAD_PREC_FP32 here) and is refused."""
    import hip_helpers as H
    import wgrad_identity as WI
    l = vad.hip.lib()
    n, h, w, cin, ncols, taps = shape
    cases = [c for c in WI.cases(l) if c[0] == shape and c[1] != 1]
    assert {c[1] for c in cases} == {0, 2, 3}
    t = torch.zeros(16, device="cuda")
    assert l.vad_conv_wgrad(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), n, h, w, cin, ncols, taps, 0 if taps == 9 else 4, 4, H.stream()) == -1
    for _, precision, form, sw in cases:
        rng = L._rng(list(shape) + [precision, 38])
        bits = 7 if precision == 3 else 23
        act, g = _data(rng, (n, h, w, cin), bits=bits), _data(rng, (n, h, w, ncols), bits=bits)

        def run(a, c):
            ad, gd = (_bf16 if precision == 3 else H.dev)(M.scaled(act, a)), (_bf16 if precision == 3 else H.dev)(M.scaled(g, c))
            ws, dw = _nan(int(l.vad_conv_wgrad_ws_floats(n, h, taps, cin, ncols))), _nan(ncols * cin * taps)
            WI.set_switches(l, sw)
            try:
                vad.hip.check(l.vad_conv_wgrad(ad.data_ptr(), gd.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, cin, ncols, taps,
                                               0 if taps == 9 else 4, precision, H.stream()))
            finally:
                WI.set_switches(l, WI.DEFAULTS)
            torch.cuda.synchronize()
            return dw.cpu().numpy()

        _equivariant(f"wgrad {shape} prec{precision} {WI.FORMS[form]} switches{sw}", _forms(l, one_cu=False), run, PAIRS)


@pytest.mark.parametrize("precision", [0, 2], ids=["fp32", "bf16op"])
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 8, 8, 32, 32), (2, 6, 10, 64, 32)])
def test_conv3x3_data_gradient_scales_exactly(vad, n, h, w, cin, cout, precision):
    """The data gradient of a 3x3 layer: vad_conv3x3 on the output gradient (2^a) with the rotated, transposed operand that
    vad_train_pack_conv3x3 writes on the device (weights 2^c); the forward operand of the same call likewise."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng = L._rng(cin + cout + h + 39)
    g, x, wt = _data(rng, (n, h, w, cout)), _data(rng, (n, h, w, cin)), _data(rng, (cout, cin, 3, 3), 0.1)

    def run(a, c):
        wd, gd, xd = H.dev(M.scaled(wt, c)), H.dev(M.scaled(g, a)), H.dev(M.scaled(x, a))
        fwd, dgr = _nan(l.vad_pack_conv3x3_floats(cout, cin)), _nan(l.vad_pack_conv3x3_floats(cin, cout))
        vad.hip.check(l.vad_train_pack_conv3x3(wd.data_ptr(), cout, cin, fwd.data_ptr(), dgr.data_ptr(), precision, H.stream()))
        zero = torch.zeros(max(cin, cout), device="cuda")
        da, out = _nan(n, h, w, cin), _nan(n, h, w, cout)
        vad.hip.check(l.vad_conv3x3(gd.data_ptr(), 0, dgr.data_ptr(), zero.data_ptr(), da.data_ptr(), 0, n, h, w, cout, cin, 0, 0, precision, H.stream()))
        vad.hip.check(l.vad_conv3x3(xd.data_ptr(), 0, fwd.data_ptr(), zero.data_ptr(), out.data_ptr(), 0, n, h, w, cin, cout, 0, 0, precision, H.stream()))
        torch.cuda.synchronize()
        return da.cpu().numpy(), out.cpu().numpy()

    _equivariant(f"conv3x3 dgrad {n}x{h}x{w} {cin}->{cout} prec{precision}", _forms(l), run, PAIRS)


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 5, 3, 128, 64), (3, 4, 4, 32, 32)])
def test_convt2x2_data_gradient_scales_exactly(vad, n, h, w, cin, cout):
    """The data gradient of a transposed convolution: vad_conv1x1 (K = 4 cout) on the space-to-depth output gradient with the
    operand vad_train_pack_convt2x2 writes; the forward operand of the same call through vad_convt2x2."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng = L._rng(cin * 3 + cout + h + 40)
    g, x, wt = _data(rng, (n, h, w, 4 * cout)), _data(rng, (n, h, w, cin)), _data(rng, (cin, cout, 2, 2), 0.1)

    def run(a, c):
        wd, gd, xd = H.dev(M.scaled(wt, c)), H.dev(M.scaled(g, a)), H.dev(M.scaled(x, a))
        fwd, dgr = _nan(l.vad_pack_convt2x2_floats(cin, cout)), _nan(l.vad_pack_conv1x1_floats(cin, 4 * cout))
        vad.hip.check(l.vad_train_pack_convt2x2(wd.data_ptr(), cin, cout, fwd.data_ptr(), dgr.data_ptr(), 0, H.stream()))
        zero = torch.zeros(max(cin, cout), device="cuda")
        da, out = _nan(n, h, w, cin), _nan(n, 2 * h, 2 * w, cout)
        vad.hip.check(l.vad_conv1x1(gd.data_ptr(), dgr.data_ptr(), zero.data_ptr(), da.data_ptr(), n * h * w, 4 * cout, cin, H.stream()))
        vad.hip.check(l.vad_convt2x2(xd.data_ptr(), 0, fwd.data_ptr(), zero.data_ptr(), out.data_ptr(), 0, n, h, w, cin, cout, 0, 0, H.stream()))
        torch.cuda.synchronize()
        return da.cpu().numpy(), out.cpu().numpy()

    _equivariant(f"convt dgrad {n}x{h}x{w} {cin}->{cout}", _forms(l), run, PAIRS)


@pytest.mark.parametrize("n,h,w,cout", [(2, 8, 8, 32), (3, 12, 20, 32), (1, 6, 6, 64)])
def test_first_layer_weight_gradient_scales_exactly(vad, n, h, w, cout):
    """vad_conv_c3_wgrad: input planes (2^a) against the output gradient (2^c)."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng = L._rng(n + h + cout + 41)
    x, g = _data(rng, (n, 3, h, w), 0.1), _data(rng, (n, h, w, cout))

    def run(a, c):
        xd, gd = H.dev(M.scaled(x, a)), H.dev(M.scaled(g, c))
        dw, ws = _nan(cout, 3, 3, 3), _nan(int(l.vad_conv_c3_wgrad_ws_floats(n, h, cout)))
        vad.hip.check(l.vad_conv_c3_wgrad(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, cout, H.stream()))
        torch.cuda.synchronize()
        return dw.cpu().numpy()

    _equivariant(f"c3 wgrad {n}x{h}x{w} ->{cout}", _forms(l, one_cu=False), run, PAIRS)


@pytest.mark.parametrize("io16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix,c", [(3 * 8 * 12, 32), (2 * 6 * 6, 64), (5 * 7 * 9, 128)])
def test_channel_sums_scale_exactly(vad, npix, c, io16):
    """vad_chan_sum / vad_chan_sum_t (bias gradients): one operand, exponents 0, +-20, +-40, +-60."""
    import hip_helpers as H
    l = vad.hip.lib()
    g = _data(L._rng(npix + c + 42), (npix, c), bits=7 if io16 else 23)

    def run(a):
        gd = (_bf16 if io16 else H.dev)(M.scaled(g, a))
        out, ws = _nan(c), _nan(max(int(l.vad_chan_ws_floats(npix, c)), 1))
        if io16:
            vad.hip.check(l.vad_chan_sum_t(gd.data_ptr(), 1, npix, c, out.data_ptr(), ws.data_ptr(), H.stream()))
        else:
            vad.hip.check(l.vad_chan_sum(gd.data_ptr(), npix, c, out.data_ptr(), ws.data_ptr(), H.stream()))
            out_t = _nan(c)
            vad.hip.check(l.vad_chan_sum_t(gd.data_ptr(), 0, npix, c, out_t.data_ptr(), ws.data_ptr(), H.stream()))
            assert torch.equal(out, out_t)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    _equivariant(f"chan_sum {npix}x{c} io16={io16}", _forms(l, one_cu=False), run, [(e,) for e in EXPONENTS])


# ============================================================================ exact statements: linear tails and metrics
def test_score_finalize_scales_exactly(vad):
    """vad_score_finalize: frame = sum(partials) / (3 H W) in a fixed order, seq = the mean over t frames - sums, one division by a
    constant, one mean.  Partial sums of squared errors are non-negative."""
    import hip_helpers as H
    parts = np.abs(_data(L._rng(43), (6, 12), 0.1))

    def run(a):
        return H.score_finalize(M.scaled(parts, a), 12, 20, t=3)

    _equivariant("score_finalize", _forms(vad.hip.lib(), one_cu=False), run, [(e,) for e in EXPONENTS])


@pytest.mark.parametrize("sigma", [1.0, 2.5])
def test_smooth_maps_scale_exactly(vad, sigma):
    """vad_smooth_maps on 3 maps of 40 x 70 (several work-group tiles, reflected borders): the smoothed maps and `frame_max`, the
    maps scaled by 2^a and the taps by 2^c.  Two passes use the taps twice: the result carries 2^(a + 2c).  Every product and sum
    is rounded on its own and a maximum is homogeneous.  Maps and taps are non-negative, so nothing cancels: every non-zero
    intermediate is at least 2^-6 times the smallest tap squared (> 2^-40) and |a + 2c| <= 60 keeps it normal."""
    import hip_helpers as H
    l = vad.hip.lib()
    r, taps = vad.metrics.gaussian_taps(sigma)
    n, h, w = 3, 40, 70
    maps = np.abs(_data(L._rng(44 + r), (n, h, w), 0.1))

    def run(a, c):
        md, td = H.dev(M.scaled(maps, a)), H.dev(M.scaled(taps, c))
        out, fmax = _nan(n, h, w), _nan(n)
        ws = torch.empty(l.vad_smooth_workspace_bytes(n, h, w, r), dtype=torch.uint8, device="cuda")
        vad.hip.check(l.vad_smooth_maps(md.data_ptr(), n, h, w, td.data_ptr(), r, out.data_ptr(), fmax.data_ptr(), ws.data_ptr(), ws.numel(), H.stream()))
        torch.cuda.synchronize()
        assert torch.equal(fmax, out.amax(dim=(1, 2)))
        return out.cpu().numpy(), fmax.cpu().numpy()

    pairs = [(0, 0), (20, 0), (-20, 0), (0, 20), (0, -20), (20, 20), (-20, -20), (40, -20)]
    assert float(taps.min()) ** 2 * 2.0 ** -6 > 2.0 ** -40
    _equivariant(f"smooth_maps sigma {sigma}", _forms(l, one_cu=False), run, pairs, exponent=lambda case: case[0] + 2 * case[1])


# ===================================================================================== split fp16: bounds against float64
# One operand v is used as hi + lo 2^-11 with hi = fp16(v), lo = fp16((v - hi) 2^11); v - hi and its scaling are exact in fp32.
#   |v| in [2^-14, 65520):  |v - hi| <= 2^-11 |v| (hi normal), lo normal or - for v a multiple of 2^-35, i.e. exponent >= -12 -
#                           exactly representable as a subnormal: |v - (hi + lo 2^-11)| <= 2^-22 |v|, |lo 2^-11| <= 2^-11 |v|.
#   |v| < 2^-14:            hi and lo sit on fp16's subnormal grid of 2^-24: |v - hi| <= 2^-25, |lo 2^11 grid| -> an ABSOLUTE
#                           representation error <= 2^-25 2^-11 = 2^-36 and |lo 2^-11| <= 2^-25 + 2^-36; below 2^-36 (exponent
#                           <= -37; round-to-even takes 2^-36 itself too) both halves are zero and the operand is gone.
#   |v| >= 65520:           hi = Inf, lo = Inf - Inf = NaN.
# A product x w is evaluated as xh wh + (xh wl + xl wh) 2^-11: fp16 x fp16 products are exact in the fp32 accumulator, the
# term xl wl 2^-22 is dropped.  With dx, dw the representation errors:
#   |error of one product| <= |dx| |w| + |x| |dw| + |dx| |dw| + |xl 2^-11| |wl 2^-11|
#     both operands in the window:  (2^-22 + 2^-22 + 2^-44 + 2^-22) |x| |w|          -> 3 * 2^-22 (1 + 2^-23) sum |x||w|
#     x below the window:           (2^-36 (1 + 2^-22) + (2^-25 + 2^-36) 2^-11) |w| + 2^-22 |x| |w|
#                                                                                    -> (2 + 2^-9) 2^-36 sum |w| + 2^-22 sum |x||w|
# and the fp32 accumulation of the 3 K terms into K-step MFMAs, the 2^-11 fold and the bias adds (K + 2) 2^-24 (sum |x||w| + |b|)
# to first order (the two correction terms are 2^-11 of the main one: their own rounding is below the second order dropped here).
# `magnitude_ref.split_bound` is the first line; `_split_B(small=...)` the second.  The issue's 3 * 2^-22 + (K + 2) 2^-24 is this
# bound with the bias magnitude added where the accumulator holds it.
SMALL = (2.0 + 2.0 ** -9) * 2.0 ** -36


def _split_B(op, x, w, k, bias_abs=0.0, small=None):
    s = M.absconv_bound(op, x, w)
    if small is None:
        return M.split_bound(s, k, bias_abs)
    gone = M.absconv_bound(op, (np.asarray(x) != 0).astype(np.float64), w) if small == "x" else M.absconv_bound(op, x, (np.asarray(w) != 0).astype(np.float64))
    return SMALL * gone + 2.0 ** -22 * s + (k + 2) * 2.0 ** -24 * (s + bias_abs)


def _ratio(tag, got, ref, bound):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == bound.shape and np.isfinite(got).all(), tag
    err = np.abs(got - ref)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"split err / B  {tag}: {worst:.3f}")
    assert worst <= 1.0, f"{tag}: |out - float64| reaches {worst:.3f} of the derived bound"
    return worst


SPLIT_LAYERS = [("conv3x3", 32, 32, 16, 16), ("conv3x3", 64, 128, 6, 10), ("convt2x2", 64, 32, 3, 5), ("convt2x2", 128, 64, 4, 4)]
#: operand shifts (a, c) that keep every exponent of bounded(-6, 1) data inside [-12, 14].  (Binade 15 is inside the window only
#: up to 65520 - a shift of 14 puts mantissas above 1.9995 past it, and the host packer says so; its top is tested at 65504.)
WINDOW = [(0, 0), (-6, -6), (13, 13), (13, -6), (-6, 13), (7, 3)]


def _split_layer(H, op, x, w, b):
    """One un-activated split-fp16 launch without BatchNorm -> NCHW fp32."""
    with L._precision(H, 1):
        return H.conv3x3(x, w, b, None, 0, False, fs=H.FS_PAD) if op == "conv3x3" else H.convt2x2(x, w, b, None, 0, fs=H.FS_PAD)


def _ref64(op, x, w, b):
    x, w, b = (torch.from_numpy(np.ascontiguousarray(v)).double() for v in (x, w, b))
    return (F.conv2d(x, w, b, padding=1) if op == "conv3x3" else F.conv_transpose2d(x, w, b, stride=2)).numpy()


def _layer_case(op, cin, cout, h, w, seed):
    rng = L._rng(cin * 1000 + cout + h + seed)
    wshape = (cout, cin, 3, 3) if op == "conv3x3" else (cin, cout, 2, 2)
    return rng, _data(rng, (3, cin, h, w)), _data(rng, wshape, 0.1), _data(rng, cout, 0.0), (9 if op == "conv3x3" else 1) * cin


@pytest.mark.parametrize("op,cin,cout,h,w", SPLIT_LAYERS)
def test_split_layers_inside_the_window(vad, op, cin, cout, h, w):
    """(a) vad_conv3x3 / vad_convt2x2 with VAD_PREC_SPLIT, operand exponents in [-12, 14]: |out - float64| <= B, B = (3 * 2^-22) S
    + (K + 2) 2^-24 (S + |b|), S = sum |x||w| (derivation above).  And the power-of-two statement bit for bit: hi is normal, lo is
    normal or an exactly representable subnormal, so the split form itself commutes with 2^k - PROVIDED the fp16 MFMA keeps
    subnormal A / B inputs and the conversions keep subnormal results (DESIGN.md records what was measured).
    Also: values 65504 (1 +- 2^-13), which still round to 65504, stay inside the same bound."""
    import hip_helpers as H
    rng, x, wt, b, k = _layer_case(op, cin, cout, h, w, 45)
    base, worst = _split_layer(H, op, x, wt, b), 0.0
    _live(op, base)
    for a, c in WINDOW:
        xs, ws, bs = M.scaled(x, a), M.scaled(wt, c), M.scaled(b, a + c)
        got = base if (a, c) == (0, 0) else _split_layer(H, op, xs, ws, bs)
        worst = max(worst, _ratio(f"{op} {cin}->{cout} {h}x{w} ({a},{c})", got, _ref64(op, xs, ws, bs), _split_B(op, xs, ws, k, np.abs(bs.astype(np.float64))[None, :, None, None])))
        _same_bits(f"{op} {cin}->{cout} split ({a},{c})", got, base, a + c)
    assert worst > 0, "split fp16 is not exact: an error of zero means the exact path ran"
    edge = x.copy()
    edge[1, 3, 2, 2], edge[0, 5, 1, 3], edge[2, 0, 0, 0] = 65504.0 * (1 + 2.0 ** -13), -65504.0 * (1 - 2.0 ** -13), 65519.0
    assert np.array_equal(torch.from_numpy(edge[[1, 0, 2], [3, 5, 0], [2, 1, 0], [2, 3, 0]]).half().float().abs().numpy(), np.full(3, 65504.0, np.float32))
    _ratio(f"{op} {cin}->{cout} inputs at 65504", _split_layer(H, op, edge, wt, b), _ref64(op, edge, wt, b), _split_B(op, edge, wt, k, np.abs(b.astype(np.float64))[None, :, None, None]))


@pytest.mark.parametrize("op,cin,cout,h,w", SPLIT_LAYERS)
def test_split_layers_above_the_window(vad, op, cin, cout, h, w):
    """(b) one input element of 2^17 in O(1) data: (hi, lo) = (Inf, NaN), so EVERY output element whose receptive field holds it is
    non-finite - never a finite number - and every other element keeps the bits of the clean launch (the masks of
    tests/test_hip_nonfinite.py: R = where the float64 reference is NaN under a NaN at the same site).  One weight of 2^17: the
    host packers refuse it (VAD_ERR_ARG naming the element); the device-side training packers cannot return an error and write
    the Inf halves - through them the kernel gives NaN on the whole footprint, and exact fp32 the ordinary finite number."""
    import hip_helpers as H
    l = vad.hip.lib()
    rng, x, wt, b, k = _layer_case(op, cin, cout, h, w, 46)
    clean = _split_layer(H, op, x, wt, b)
    for label, idx in NF._x_sites(x):
        for value in (2.0 ** 17, -2.0 ** 17, 65520.0):
            bad = x.copy()
            bad[idx] = value
            foot = np.isnan(_ref64(op, NF._put(x, idx, "+nan"), wt, b))
            assert foot[1].any() and not foot[1].all() and not foot[[0, 2]].any()
            got = _split_layer(H, op, bad, wt, b)
            assert not np.isfinite(got[foot]).any(), f"{op} {label} {value}: {int(np.isfinite(got[foot]).sum())} finite elements inside the footprint"
            assert NF._bits_equal(got, clean, ~foot), f"{op} {label} {value}: an element outside the footprint changed"
            with L._precision(H, 0):
                exact = H.conv3x3(bad, wt, b, None, 0, False) if op == "conv3x3" else H.convt2x2(bad, wt, b, None, 0)
            assert np.isfinite(exact).all() and np.abs(exact - _ref64(op, bad, wt, b)).max() < 2.0 ** -20 * 2.0 ** 19
    widx = (1, cin // 2, 1, 1) if op == "conv3x3" else (cin // 2, 1, 0, 1)
    bad = wt.copy()
    bad[widx] = 2.0 ** 17
    with pytest.raises(H.hip.VadError, match=r"split precision cannot hold folded weight .* = 131072 "):
        _split_layer(H, op, x, bad, b)
    foot = np.isnan(_ref64(op, x, NF._put(wt, widx, "+nan"), b))
    assert foot.any() and not foot.all()
    wd, bd = H.dev(bad), H.dev(b)
    xin = H._in_frames(x, None)
    if op == "conv3x3":
        fwd, out = _nan(l.vad_pack_conv3x3_floats(cout, cin)), H._out_frames(3, (h, w, cout), None)
        vad.hip.check(l.vad_train_pack_conv3x3(wd.data_ptr(), cout, cin, fwd.data_ptr(), None, 1, H.stream()))
        vad.hip.check(l.vad_conv3x3(xin.ptr, 0, fwd.data_ptr(), bd.data_ptr(), out.ptr, 0, 3, h, w, cin, cout, 0, 0, 1, H.stream()))
    else:
        fwd, out = _nan(l.vad_pack_convt2x2_floats(cin, cout)), H._out_frames(3, (2 * h, 2 * w, cout), None)
        vad.hip.check(l.vad_train_pack_convt2x2(wd.data_ptr(), cin, cout, fwd.data_ptr(), None, 1, H.stream()))
        vad.hip.check(l.vad_convt2x2(xin.ptr, 0, fwd.data_ptr(), bd.data_ptr(), out.ptr, 0, 3, h, w, cin, cout, 0, 1, H.stream()))
    got = H._result(out)
    assert not np.isfinite(got[foot]).any() and NF._bits_equal(got, clean, ~foot)


@pytest.mark.parametrize("op,cin,cout,h,w", SPLIT_LAYERS)
def test_split_layers_below_the_window(vad, op, cin, cout, h, w):
    """(c) one operand with every exponent at -20, -30 or -45, the other O(1).  -20: hi is a subnormal fp16; -30: hi = 0 and the
    value lives in a subnormal lo.  Either way the operand is held on fp16's subnormal grid - an absolute representation error of
    2^-36 in place of 2^-22 |v| - and the error stays within (2 + 2^-9) 2^-36 sum |w| + 2^-22 S + (K + 2) 2^-24 (S + |b|).  That
    bound holds only if the fp16 MFMA and the conversions KEEP subnormals (a flush would lose the operand: an error of |x||w|,
    2^15 times the bound at -20).  -45: both halves are zero, the operand is gone and the output is the bias, bit for bit."""
    import hip_helpers as H
    rng, x, wt, b, k = _layer_case(op, cin, cout, h, w, 47)
    ba = np.abs(b.astype(np.float64))[None, :, None, None]
    for which in ("x", "w"):
        for e in (-20, -30, -45):
            xs = M.bounded(rng, x.shape, e, e, 0.3) if which == "x" else x
            ws = M.bounded(rng, wt.shape, e, e, 0.1) if which == "w" else wt
            got = _split_layer(H, op, xs, ws, b)
            tag = f"{op} {cin}->{cout} {which} at 2^{e}"
            if e == -45:
                assert np.array_equal(got, np.broadcast_to(b[None, :, None, None], got.shape)), f"{tag}: the output is not the bias alone"
                continue
            r = _ratio(tag, got, _ref64(op, xs, ws, b), _split_B(op, xs, ws, k, ba, small=which))
            lost = np.abs(_ref64(op, xs, ws, b) - b[None, :, None, None].astype(np.float64)).max()
            assert r <= 1.0 and lost > 4 * np.max(_split_B(op, xs, ws, k, 0.0, small=which)), tag       # a vanished operand would be noticed


@pytest.mark.parametrize("h,w", [(16, 16), (22, 18)])
def test_split_fused_enc1_block(vad, h, w):
    """vad_conv3x3_c3_fused with VAD_PREC_SPLIT, both stages.  The first stage's result is data of the second whose exponents are
    not ours to bound (a value below 2^-14 is held to 2^-36 absolute, not 2^-22 relative), so with mid = LeakyReLU(conv0) in float64
      E0 = B(x, w0, K = 32, b0) + 2^-24 |mid|                                                (stage 1 + the rounding of 0.2 y)
      B  = sum |w1| E0 + 3 * 2^-22 S1 + (2 + 2^-9) 2^-36 sum |w1| + 290 * 2^-24 (S1 + |b1|) + 2^-24 |out|,  S1 = sum (|mid| + E0) |w1|
    (LeakyReLU and max-pooling are 1-Lipschitz; pooling takes the largest bound of its window).  (a) inside the window for the
    inputs and both weights, (b) one input pixel of 2^17: its whole footprint is non-finite, everything else keeps its bits, (c) the
    inputs at exponent -20 and -30 under the absolute form of E0.  The bit-for-bit statement is left to the single layers: the data
    do not allow it here."""
    import hip_helpers as H
    rng = L._rng(h * 100 + w + 48)
    x = _data(rng, (3, 3, h, w), 0.1)
    w0, b0, w1, b1 = _data(rng, (32, 3, 3, 3), 0.0), _data(rng, 32, 0.0), _data(rng, (32, 32, 3, 3), 0.1), _data(rng, 32, 0.0)

    def run(x, w0, b0, w1, b1):
        with L._precision(H, 1):
            return H.conv3x3_c3_fused(x, w0, b0, None, w1, b1, None)

    def ref_and_bound(x, w0, b0, w1, b1, small=None):
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
        b0a, b1a = (np.abs(v.astype(np.float64))[None, :, None, None] for v in (b0, b1))
        mid = F.leaky_relu(F.conv2d(t(x), t(w0), t(b0), padding=1), 0.2)
        e0 = _split_B("conv3x3", x, w0, 32, b0a, small=small) + 2.0 ** -24 * mid.abs().numpy()
        pre = F.leaky_relu(F.conv2d(mid, t(w1), t(b1), padding=1), 0.2)
        s1 = M.absconv_bound("conv3x3", mid.abs().numpy() + e0, w1)
        bound = M.absconv_bound("conv3x3", e0, w1) + 3.0 * 2.0 ** -22 * s1 + SMALL * M.absconv_bound("conv3x3", np.ones_like(e0), w1) \
            + 290 * 2.0 ** -24 * (s1 + b1a) + 2.0 ** -24 * pre.abs().numpy()
        return F.max_pool2d(pre, 2, 2).numpy(), F.max_pool2d(torch.from_numpy(bound), 2, 2).numpy()

    clean = run(x, w0, b0, w1, b1)
    _live("fused", clean)
    worst = 0.0
    # (|mid| <= 27 * 16 + 4 < 2^9 at (0, 0): a + c0 <= 6 keeps the intermediate inside the window too)
    for a, c0, c1 in [(0, 0, 0), (-6, -6, 0), (6, -6, 0), (-6, 6, -6), (3, 3, 3), (0, 0, 13)]:
        args = (M.scaled(x, a), M.scaled(w0, c0), M.scaled(b0, a + c0), M.scaled(w1, c1), M.scaled(b1, a + c0 + c1))
        worst = max(worst, _ratio(f"c3_fused {h}x{w} ({a},{c0},{c1})", clean if (a, c0, c1) == (0, 0, 0) else run(*args), *ref_and_bound(*args)))
    assert worst > 0
    for label, idx in NF._x_sites(x):
        bad = x.copy()
        bad[idx] = 2.0 ** 17
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
        mid = F.leaky_relu(F.conv2d(t(NF._put(x, idx, "+nan")), t(w0), t(b0), padding=1), 0.2)
        foot = np.isnan(F.max_pool2d(F.leaky_relu(F.conv2d(mid, t(w1), t(b1), padding=1), 0.2), 2, 2).numpy())
        assert foot[1].any() and not foot[[0, 2]].any()
        got = run(bad, w0, b0, w1, b1)
        assert not np.isfinite(got[foot]).any(), f"fused {label}: finite elements inside the footprint of an input of 2^17"
        assert NF._bits_equal(got, clean, ~foot), f"fused {label}: an element outside the footprint changed"
    for e in (-20, -30):
        xs = M.bounded(rng, x.shape, e, e, 0.1)
        _ratio(f"c3_fused {h}x{w} x at 2^{e}", run(xs, w0, b0, w1, b1), *ref_and_bound(xs, w0, b0, w1, b1, small="x"))


@pytest.mark.parametrize("shape", __import__("wgrad_identity").SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_weight_gradient_forms(vad, shape):
    """vad_conv_wgrad with VAD_PREC_SPLIT in its per-lane, LDS-staged and row-ring forms (vad_debug_set_wgrad_split 1, 2, 3; a form
    that does not take the shape falls through to the next lower one), K = N H W pixels, no bias.  (a) |dW - float64| <= B and
    the bit-for-bit power-of-two statement inside the window; (b) one activation of 2^17: every weight-gradient element that
    sums it is non-finite, all others keep their bits; (c) the activations at exponent -20 / -30 within the absolute form of the
    bound, at -45 gone: dW = 0."""
    import hip_helpers as H
    l = vad.hip.lib()
    n, h, w, cin, ncols, taps = shape
    rng = L._rng(list(shape) + [49])
    act, g = _data(rng, (n, cin, h, w)), _data(rng, (n, ncols, h, w))
    op, k = ("wgrad3x3" if taps == 9 else "wgrad1x1"), n * h * w
    dshape = (ncols, cin, 3, 3) if taps == 9 else (ncols, cin, 1, 1)

    def ref64(a_, g_):
        a64, g64 = torch.from_numpy(a_).double(), torch.from_numpy(g_).double()
        if taps == 1:
            return torch.einsum("nchw,nohw->oc", a64, g64)[:, :, None, None].numpy()
        cols = F.unfold(a64, 3, padding=1).view(n, cin, 9, h * w)
        return torch.einsum("nckp,nop->ock", cols, g64.reshape(n, ncols, h * w)).reshape(dshape).numpy()

    def run(mode, a_, g_):
        ad, gd = H.nhwc(a_), H.nhwc(g_)
        ws, dw = _nan(int(l.vad_conv_wgrad_ws_floats(n, h, taps, cin, ncols))), _nan(*dshape)
        l.vad_debug_set_wgrad_split(mode)
        try:
            vad.hip.check(l.vad_conv_wgrad(ad.data_ptr(), gd.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, cin, ncols, taps, 0 if taps == 9 else 4, 1, H.stream()))
        finally:
            l.vad_debug_set_wgrad_split(3)
        torch.cuda.synchronize()
        return dw.cpu().numpy()

    for mode in (1, 2, 3):
        base, worst = run(mode, act, g), 0.0
        _live(f"wgrad mode {mode}", base)
        for a, c in WINDOW:
            as_, gs = M.scaled(act, a), M.scaled(g, c)
            got = base if (a, c) == (0, 0) else run(mode, as_, gs)
            worst = max(worst, _ratio(f"wgrad {shape} form {mode} ({a},{c})", got, ref64(as_, gs), _split_B(op, as_, gs, k)))
            _same_bits(f"wgrad {shape} split form {mode} ({a},{c})", got, base, a + c)
        assert worst > 0
        idx = (1, cin // 2, NF._odd(h), NF._odd(w))
        bad = act.copy()
        bad[idx] = 2.0 ** 17
        foot = np.isnan(ref64(NF._put(act, idx, "+nan"), g))
        assert foot.any() and not foot.all()
        got = run(mode, bad, g)
        assert not np.isfinite(got[foot]).any(), f"wgrad {shape} form {mode}: finite elements where an activation of 2^17 is summed"
        assert NF._bits_equal(got, base, ~foot), f"wgrad {shape} form {mode}: an element outside the footprint changed"
        for e in (-20, -30, -45):
            as_ = M.bounded(rng, act.shape, e, e, 0.3)
            got = run(mode, as_, g)
            if e == -45:
                assert not got.any(), f"wgrad {shape} form {mode}: activations at 2^-45 still reach dW"
            else:
                _ratio(f"wgrad {shape} form {mode} activations at 2^{e}", got, ref64(as_, g), _split_B(op, as_, g, k, small="x"))


# ================================================================================================ models (Python surface)
def _np(out):
    return {k: v for k, v in out.items() if torch.is_tensor(v)}


def _models(vad):
    return {
        "image": ("image", lambda: vad.ConvAutoencoder(in_channels=3, latent_dim=32), (3, 3, 32, 32)),
        "image-c5": ("image", lambda: vad.ConvAutoencoder(in_channels=5, latent_dim=32), (3, 5, 32, 32)),
        "video-1": ("video", lambda: vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1), (2, 3, 3, 32, 32)),
        "video-2": ("video", lambda: vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=2), (2, 3, 3, 32, 32)),
    }


def _inputs(vad, name, shape):
    """[(label, device tensor)]: float frames / clips from the synthetic generator, and - 3-channel image model - the same as uint8."""
    if len(shape) == 5:
        x = vad.synth.clips(61, 0, shape[0], shape[1], shape[2], shape[3], shape[4])
    else:
        x = vad.synth.frames(62, 0, shape[0], shape[1], shape[2], shape[3])
    out = [("float", torch.from_numpy(x).cuda())]
    if name == "image":
        u8 = np.clip(np.round((x * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()
        out.append(("uint8", torch.from_numpy(u8).cuda()))
    return x, out


def _oracle(kind, st, x, layers):
    s = {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}
    return torch_oracle.img_scores(s, torch.from_numpy(x)) if kind == "image" else torch_oracle.vid_scores(s, torch.from_numpy(x), 32, layers)


def _against_oracle(tag, kind, out, ref):
    for k in (("scores",) if kind == "image" else ("frame", "seq")):
        assert rel_err(out[k].cpu().numpy(), ref[k].numpy()) < 1e-5, (tag, k)
    assert np.abs(out["recon"].cpu().numpy() - ref["recon"].numpy()).max() < 5e-5, tag


@pytest.mark.parametrize("precision", ["fp32", "winograd"])
@pytest.mark.parametrize("name", ["image", "image-c5", "video-1", "video-2"])
def test_rebalanced_models_score_identically(vad, name, precision):
    """`score_all` of a rebalanced model (magnitude_ref.rebalance: BatchNorm weight and bias times 2^s, the next convolution's
    input channels times 2^-s) is torch.equal to the base model's in every output - scores, error map, reconstruction, frame and
    sequence scores - for each single boundary at +-40 and for alternating +-20 at all of them: the activations between two
    layers move by up to 2^40, no bit of any product does.  Image models under both vad_debug_set_dec4_fused settings (the two
    boundaries inside the fused enc1 and the fused dec4 launch), float and uint8 frames.  One rebalanced model per kind is also
    held to the float oracle on its OWN state dict at the fuzz test's bounds, which ties the statement to the reference."""
    l = vad.hip.lib()
    kind, make, shape = _models(vad)[name]
    m = make()
    st = load_synthetic(vad, m, 63)
    m = m.cuda().eval()
    m.precision = precision
    x, inputs = _inputs(vad, name, shape)
    nb = len(M.boundaries(st, kind))
    plans = [{j: s} for j in range(nb) for s in (40, -40)] + [M.alternating(nb, 20), M.alternating(nb, -20)]
    try:
        for fused in ((1, 0) if kind == "image" else (1,)):
            l.vad_debug_set_dec4_fused(fused)
            NF._load(m, st)
            with torch.no_grad():
                base = [_np(m.score_all(t)) for _, t in inputs]
            assert all(torch.isfinite(v).all() for b in base for v in b.values())
            if fused:
                _against_oracle(f"{name} {precision} base", kind, base[0], _oracle(kind, st, x, 2 if name == "video-2" else 1))
            for shifts in plans:
                re = M.rebalance(st, kind, shifts)
                NF._load(m, re)
                with torch.no_grad():
                    for (label, t), b in zip(inputs, base):
                        got = _np(m.score_all(t))
                        assert sorted(got) == sorted(b)
                        for k in b:
                            assert torch.equal(got[k], b[k]), f"{name} {precision} fused={fused} {label} shifts {shifts}: {k} differs from the base model's"
                if fused and shifts is plans[-2]:
                    _against_oracle(f"{name} {precision} rebalanced", kind, got, _oracle(kind, re, x, 2 if name == "video-2" else 1))
    finally:
        l.vad_debug_set_dec4_fused(1)
        NF._load(m, st)


def _split_scores(m, kind, t):
    """-> frame-level scores as numpy, or None when the packer refused the state (split precision cannot hold a folded weight)."""
    import importlib
    hip = importlib.import_module("video-anomaly-detection_amd.hip")
    try:
        with torch.no_grad():
            out = m.score_all(t)
    except hip.VadError as e:
        assert "split precision cannot hold folded weight" in str(e) and "layer " in str(e), str(e)
        return None
    return out["scores" if kind == "image" else "frame"].cpu().numpy()


@pytest.mark.parametrize("name", ["image", "image-c5", "video-1", "video-2"])
def test_split_models_inside_and_outside_the_window(vad, name):
    """precision = "split" through the Python surface.
      * alternating shifts of +-4 and +-8 at every boundary keep the mode's gate: scores within 1e-5 relative of the oracle on
        the rebalanced state dict;
      * +20 at any single boundary never gives a finite wrong score.  The shift lands in the folded weights of the layer in FRONT
        of the boundary (refused by the packer, VadError naming the layer) and in the activations behind it (2^20: Inf halves, NaN
        scores for every frame).  One boundary is neither: ConvAutoencoder's last one (dec4.1 -> dec4.3) lies between two layers
        that are exact fp32 in every blob (dec4_fused.hip), so the scores are finite AND right - held to the same 1e-5;
      * +16 at the first boundary alone keeps every folded weight of the first layer below 65520 - the blob packs - while the
        activations behind it pass 65504: NaN scores for every frame."""
    kind, make, shape = _models(vad)[name]
    m = make()
    st = load_synthetic(vad, m, 64)
    m = m.cuda().eval()
    m.precision = "split"
    x, inputs = _inputs(vad, name, shape)
    layers = 2 if name == "video-2" else 1
    nb = len(M.boundaries(st, kind))
    key = "scores" if kind == "image" else "frame"
    try:
        for s in (4, -4, 8, -8):
            re = M.rebalance(st, kind, M.alternating(nb, s))
            NF._load(m, re)
            got = _split_scores(m, kind, inputs[0][1])
            assert got is not None, f"{name}: alternating {s} was refused"
            err = rel_err(got, _oracle(kind, re, x, layers)[key].numpy())
            print(f"split {name} alternating {s:+d}: scores rel err {err:.3e}")
            assert err < 1e-5, (name, s, err)
        refused = nan = 0
        for j in range(nb):
            re = M.rebalance(st, kind, {j: 20})
            NF._load(m, re)
            for label, t in inputs:
                got = _split_scores(m, kind, t)
                if got is None:
                    refused += 1
                elif name in ("image",) and j == nb - 1:
                    assert rel_err(got, _oracle(kind, re, x, layers)[key].numpy()) < 1e-5, (name, j, label)
                else:
                    assert np.isnan(got).all(), f"{name} +20 at boundary {j} ({label}): scores {got}"
                    nan += 1
        print(f"split {name} +20 at one boundary: {refused} refused, {nan} all-NaN")
        re = M.rebalance(st, kind, {0: 16})
        NF._load(m, re)
        for label, t in inputs:
            got = _split_scores(m, kind, t)
            assert got is not None, f"{name}: +16 at the first boundary was refused - the case needs packable weights"
            assert np.isnan(got).all(), f"{name} +16 at the first boundary ({label}): scores {got}"
    finally:
        NF._load(m, st)
