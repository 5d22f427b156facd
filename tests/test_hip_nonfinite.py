"""GPU tests of the non-finite contract ("Non-finite values"): a NaN is never erased, an Inf never becomes a finite
value the reference would not produce, and in eval mode a non-finite value in one frame changes no bit of another frame.

Every case runs the operation on clean seeded data, poisons ONE element (+NaN 0x7FC00000, -NaN 0xFFC00000, +Inf, -Inf) and
runs it again.  The reference is the same operation composed from torch CPU operators in float64 on the same data (not the C
oracle).  F = the output elements the float64 reference makes differ from its own clean run; R = the elements whose receptive
field holds the poisoned element (= where the reference is NaN under the +NaN poison at the same site).

  * input poisons sit in frame 1 of three: F is neither empty nor the whole frame (no vacuous pass), frames 0 and 2 are bitwise
    equal to the clean run;
  * every element outside the mask is bitwise equal to the clean run.  The mask is F, except
      - Winograd kernels: F widened to the 2x2 output tiles whose 4x4 input tile holds the poisoned element (their input
        transform mixes the tile - that much and no more);
      - split-fp16 and Winograd under an Inf poison: R.  Inf splits into (hi, lo) = (Inf, Inf - Inf = NaN), and the Winograd
        transforms form Inf - Inf, so inside R these two may be non-finite where the reference is finite (and where it equals
        its clean value, e.g. ReLU(-Inf) = 0).  Outside R nothing may move.
  * NaN poison: the reference is NaN on exactly F, the kernel is NaN on all of F;
  * Inf poison: wherever the reference is non-finite the kernel is non-finite; where it is finite inside F the exact-fp32 direct
    kernels give the reference's value to the layer tests' ATOL (split / Winograd: that value or a non-finite one).

  * two 0 * Inf sites remain in exact-fp32 kernels, both inside R and both turning an Inf into a NaN, never into a finite value
    (a NaN poison is unaffected: every element concerned has the poisoned one in its receptive field anyway):
      - the first-layer kernels (vad_conv3x3_c3, the fused enc1 block) pad K = 27 to 28 with a ZERO WEIGHT against the tile
        value of tap (channel 0, dy 0, dx 0): an Inf in channel 0 at (y, x) gives NaN in the one output pixel (y + 1, x + 1),
        every channel, where the reference has +-Inf or ReLU(-Inf) = 0;
      - vad_conv3x3_to3_score (the image tail when the fused dec4 kernel is switched off) pads by multiplying a clamped, i.e.
        in-frame, border row / column with 0: an Inf in the first or last row / column of its input map makes the border
        outputs beside it NaN where the reference has tanh(+-Inf) = +-1.
    These elements (`nan_ok`) may be NaN under an Inf poison; everything else holds for these kernels as for the others.

No case derives an address from poisoned data."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_hip_layers as L
from conftest import load_synthetic
from oracle import torch_oracle

pytestmark = pytest.mark.gpu

ATOL = L.ATOL            # 3e-5, the layer tests' bound
LSTM_ATOL = 2e-5         # the ConvLSTM step's
POISONS = {"+nan": 0x7FC00000, "-nan": 0xFFC00000, "+inf": 0x7F800000, "-inf": 0xFF800000}
NANS = ("+nan", "-nan")


@pytest.fixture(autouse=True)
def _fixed_cpu_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(before)


def _put(a, idx, poison):
    """A C-contiguous fp32 copy of `a` with the poison's BIT PATTERN at idx (an assignment of a float may drop a NaN's sign)."""
    out = np.array(a, dtype=np.float32, order="C")
    out.view(np.uint32)[idx] = POISONS[poison]
    return out


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _bits_equal(a, b, where=None):
    a, b = np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
    return np.array_equal(a, b) if where is None else np.array_equal(a[where], b[where])


def _check(tag, poison, got_c, got_p, ref_c, ref_p, ref_nan, exact, atol=ATOL, widen=None, frame=None, nan_ok=None):
    """The assertions of the module docstring for one output tensor (leading axis = frames).  ref_nan: the reference under the
    +NaN poison at the same site; frame: the poisoned input frame (None: a parameter was poisoned, every frame may change);
    nan_ok: elements (inside R) where an exact kernel may give NaN under an Inf poison - the 0 * Inf sites of the docstring."""
    got_c, got_p = np.ascontiguousarray(got_c, np.float32), np.ascontiguousarray(got_p, np.float32)
    assert got_p.shape == ref_p.shape == got_c.shape, tag
    assert np.isfinite(got_c).all() and np.isfinite(ref_c).all(), tag
    Fm = ~(ref_p == ref_c)
    R = np.isnan(ref_nan)
    assert Fm.any(), f"{tag}: the poison reaches no output element of the reference (vacuous case)"
    if frame is not None:
        others = [i for i in range(len(Fm)) if i != frame]
        assert not Fm[frame].all(), f"{tag}: the footprint is the whole frame (vacuous isolation check)"
        assert not Fm[others].any(), tag
        assert _bits_equal(got_p[others], got_c[others]), f"{tag}: another frame changed"
    nan = poison in NANS
    mask = Fm if (exact or nan) else (Fm | R)
    if widen is not None:
        mask = mask | widen
    if nan_ok is not None and not nan:
        assert not (nan_ok & ~R).any(), tag
        mask = mask | nan_ok
    moved = ~mask & (got_p.view(np.uint32) != got_c.view(np.uint32))
    assert not moved.any(), f"{tag}: {int(moved.sum())} elements outside the footprint changed, first at {tuple(np.argwhere(moved)[0])}"
    if nan:
        assert np.array_equal(np.isnan(ref_p), Fm), tag
        lost = Fm & ~np.isnan(got_p)
        assert not lost.any(), f"{tag}: {int(lost.sum())} of {int(Fm.sum())} NaN elements erased, first at {tuple(np.argwhere(lost)[0])} = {got_p[lost][0]!r}"
        return
    nf = ~np.isfinite(ref_p)
    lost = nf & np.isfinite(got_p)
    assert not lost.any(), f"{tag}: {int(lost.sum())} non-finite elements of the reference are finite, first at {tuple(np.argwhere(lost)[0])} = {got_p[lost][0]!r}"
    fin = Fm & ~nf
    with np.errstate(invalid="ignore"):
        close = np.abs(got_p.astype(np.float64) - ref_p) < atol
    ok = close | (~fin) if exact else (close | ~np.isfinite(got_p) | ~fin)
    if nan_ok is not None:
        ok = ok | (nan_ok & np.isnan(got_p))
    assert ok.all(), f"{tag}: {int((~ok).sum())} finite elements inside the footprint are off, first at {tuple(np.argwhere(~ok)[0])}: {got_p[~ok][0]!r} vs {ref_p[~ok][0]!r}"


def _odd(k):
    """An interior odd coordinate: the bottom / right element of its pooling window."""
    return 3 if k > 4 else 1


def _x_sites(x, frame=1):
    n, c, h, w = x.shape
    return [("x-interior", (frame, c // 2, _odd(h), _odd(w))), ("x-first", (frame, 0, 0, 0)), ("x-last", (frame, c - 1, h - 1, w - 1))]


class _plan_cus:
    def __init__(self, l, cus):
        self.l, self.cus = l, cus

    def __enter__(self):
        self.l.vad_debug_set_plan_cus(self.cus)

    def __exit__(self, *exc):
        self.l.vad_debug_set_plan_cus(0)


class _variant:
    def __init__(self, l, bits):
        self.l, self.bits = l, bits

    def __enter__(self):
        self.l.vad_debug_set_conv_variant(self.bits)

    def __exit__(self, *exc):
        self.l.vad_debug_set_conv_variant(1)


def _forms(l, run, variants=(1 | 64, 1 | 128, 0), one_cu=True):
    """{label: callable} - `run` under the default plan, every kernel-form switch and the one-CU plan (persistent walks)."""
    def under(ctx):
        def call(**args):
            with ctx:
                return run(**args)
        return call
    forms = {"default": run}
    for bits in variants:
        forms[f"variant{bits}"] = under(_variant(l, bits))
    if one_cu:
        forms["one-cu"] = under(_plan_cus(l, 1))
    return forms


def _sweep(tag, forms, ref, args, sites, exact, atol=ATOL, widen=None, poisons=tuple(POISONS), outputs=1, nan_ok=None):
    """args: dict of named fp32 arrays; sites: [(label, key, index, frame | None)]; ref(**args) -> float64 array (or a tuple of
    `outputs` arrays); forms: {label: run(**args) -> fp32 array (or tuple)}.  widen(label, index, shape) -> bool mask | None."""
    def tup(v):
        return v if isinstance(v, tuple) else (v,)
    ref_c = tup(ref(**args))
    got_c = {k: tup(run(**args)) for k, run in forms.items()}
    for label, key, idx, frame in sites:
        ref_nan = tup(ref(**{**args, key: _put(args[key], idx, "+nan")}))
        for poison in poisons:
            pa = {**args, key: _put(args[key], idx, poison)}
            ref_p = ref_nan if poison == "+nan" else tup(ref(**pa))
            for fname, run in forms.items():
                got_p = tup(run(**pa))
                for o in range(outputs):
                    wd = widen(label, idx, ref_p[o].shape) if widen is not None else None
                    nk = nan_ok(label, idx, ref_p[o].shape) if nan_ok is not None else None
                    _check(f"{tag} {label}{idx} {poison} {fname} out{o}", poison, got_c[fname][o], got_p[o], ref_c[o], ref_p[o], ref_nan[o],
                           exact, atol, wd, frame, nk)


# ------------------------------------------------------------------------------------------------- float64 references
def _act64(y, act):
    return F.leaky_relu(y, 0.2) if act == 1 else (F.relu(y) if act == 2 else y)


def _bn64(y, bn):
    if bn is None:
        return y
    g, b, m, v = (_t64(a) for a in bn)
    return F.batch_norm(y, m, v, g, b, training=False, eps=1e-5)


def _ref_conv(x, w, b, bn, act, pool, pad=1):
    y = _act64(_bn64(F.conv2d(_t64(x), _t64(w), _t64(b), padding=pad), bn), act)
    return (F.max_pool2d(y, 2, 2) if pool else y).numpy()


def _ref_convt(x, w, b, bn, act):
    return _act64(_bn64(F.conv_transpose2d(_t64(x), _t64(w), _t64(b), stride=2), bn), act).numpy()


def _c3_pad_tap(label, idx, shape, div, grow):
    """The first-layer kernels' K-padding tap (module docstring): for an x poison in channel 0 at (y, x) the output pixel
    (y + 1, x + 1), grown by `grow` pixels (a 3x3 convolution behind it) and divided by `div` (pooling), all channels."""
    if not label.startswith("x-") or idx[1] != 0:
        return None
    f, _, y, x = idx
    m = np.zeros(shape, bool)
    m[f, :, max(0, y + 1 - grow) // div:(y + 1 + grow) // div + 1, max(0, x + 1 - grow) // div:(x + 1 + grow) // div + 1] = True
    return m


def _param_sites(w_idx, cout, bn=True):
    """One weight element (the centre tap for a 3x3: no zero padding ever meets it), one bias, one folded BatchNorm beta."""
    s = [("weight", "w", w_idx, None), ("bias", "b", (2,), None)]
    return s + ([("beta", "beta", (cout - 1,), None)] if bn else [])


# --------------------------------------------------------------------------------------------------------- conv3x3
@pytest.mark.parametrize("cin,cout,h,w,act,pool,precision", L._with_precision(
    [(cin, cout, h, w, act, pool) for (cin, cout, h, w) in [(3, 32, 16, 16), (32, 32, 16, 16), (64, 64, 8, 12), (128, 128, 6, 10)]
     for act in (1, 2) for pool in (False, True)], split=lambda case: case[0] != 3))
def test_conv3x3(cin, cout, h, w, act, pool, precision):
    """vad_conv3x3 / vad_conv3x3_c3.  Sites reached: vad_act's ReLU / LeakyReLU in every epilogue; the pooling maxima of
    conv_pkernel.h (default plan and one-CU plan, variant 1|64: persistent 32x32x2), conv_small.h (variant 1|128: the gate-split
    small-grid kernel, pooled and un-pooled epilogue), conv_mfma.hip's one-tile kernel (variant 0) and first-layer kernels
    (cin 3: conv3x3_c3_kernel under variant 0, the persistent first layer otherwise).  The interior poison sits at an odd row and
    column: it is one of four in its pooling window, where the old maxima kept a NaN only if all four were NaN.
    Split precision and Inf: see the module docstring (non-finite allowed inside R only)."""
    import hip_helpers as H
    l = H.hip.lib()
    rng = L._rng(cin * 1000 + cout + h + 11)
    x = rng.standard_normal((3, cin, h, w)).astype(np.float32)
    wt, b, bn = L._conv_params(rng, cout, cin)
    args = {"x": x, "w": wt, "b": b, "beta": bn[1]}

    def run(x, w, b, beta):
        with L._precision(H, precision):
            return H.conv3x3(x, w, b, [bn[0], beta, bn[2], bn[3]], act, pool)

    def ref(x, w, b, beta):
        return _ref_conv(x, w, b, [bn[0], beta, bn[2], bn[3]], act, pool)

    sites = [(s, "x", i, 1) for s, i in _x_sites(x)] + _param_sites((1, cin // 2, 1, 1), cout)
    forms = _forms(l, run) if precision == 0 else _forms(l, run, variants=())
    nan_ok = (lambda label, idx, shape: _c3_pad_tap(label, idx, shape, 2 if pool else 1, 0)) if cin == 3 else None
    _sweep(f"conv3x3 {cin}->{cout} {h}x{w} act{act} pool{int(pool)} prec{precision}", forms, ref, args, sites, exact=precision == 0, nan_ok=nan_ok)


def _wino_widen(label, idx, shape, pool):
    """F(2x2,3x3): output tile (ty, tx) = output rows 2ty, 2ty+1 from input rows 2ty-1 .. 2ty+2 (tiles start at row / column 0).
    -> the outputs (pooled: the one output) of every tile whose 4x4 input tile holds input element idx, all channels."""
    if not label.startswith("x-"):
        return None
    f, _, y, x = idx
    m = np.zeros(shape, bool)
    for ty in range(max(0, (y - 1) // 2), (y + 1) // 2 + 1):
        for tx in range(max(0, (x - 1) // 2), (x + 1) // 2 + 1):
            if pool:
                m[f, :, ty:ty + 1, tx:tx + 1] = True
            else:
                m[f, :, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = True
    return m


@pytest.mark.parametrize("cin,cout,h,w,act,pool", [(32, 32, 16, 16, 1, False), (32, 32, 16, 16, 2, True), (32, 32, 16, 16, 1, True),
                                                    (32, 32, 16, 16, 2, False), (64, 64, 5, 9, 1, False), (64, 64, 5, 9, 2, False)])
def test_conv3x3_wino(cin, cout, h, w, act, pool):
    """vad_conv3x3_wino (conv_wino.hip: the pooling maximum of its epilogue and vad_act behind it; 5x9 has partial tiles, where
    pooling is refused).  The input transform mixes a 4x4 tile, so the mask is F widened to the tiles that hold the poisoned
    element; under an Inf poison the transforms form Inf - Inf and the tile's outputs may be NaN where the reference is
    finite (module docstring)."""
    import hip_helpers as H
    l = H.hip.lib()
    rng = L._rng(cin * 1000 + cout + h + 12)
    x = rng.standard_normal((3, cin, h, w)).astype(np.float32)
    wt, b, bn = L._conv_params(rng, cout, cin)
    args = {"x": x, "w": wt, "b": b, "beta": bn[1]}
    run = lambda x, w, b, beta: H.conv3x3_wino(x, w, b, [bn[0], beta, bn[2], bn[3]], act, pool)
    ref = lambda x, w, b, beta: _ref_conv(x, w, b, [bn[0], beta, bn[2], bn[3]], act, pool)
    sites = [(s, "x", i, 1) for s, i in _x_sites(x)] + _param_sites((1, cin // 2, 1, 1), cout)
    _sweep(f"wino {cin}->{cout} {h}x{w} act{act} pool{int(pool)}", _forms(l, run, variants=()), ref, args, sites, exact=False,
           widen=lambda label, idx, shape: _wino_widen(label, idx, shape, pool))


@pytest.mark.parametrize("h,w,precision", L._with_precision([(16, 16), (22, 18)]))
def test_conv3x3_c3_fused(h, w, precision):
    """The fused enc1 block (conv 3->32 + LeakyReLU in the tile, conv 32->32 + LeakyReLU + pooling: conv_mfma.hip's fused
    staging and the pooled epilogues of the persistent and - variant 0 - the one-tile kernel).  Receptive field 5x5 + pooling."""
    import hip_helpers as H
    l = H.hip.lib()
    rng = L._rng(h * 100 + w + 13)
    x = rng.uniform(-1, 1, (3, 3, h, w)).astype(np.float32)
    w0, b0, bn0 = L._conv_params(rng, 32, 3)
    w1, b1, bn1 = L._conv_params(rng, 32, 32)
    args = {"x": x, "w0": w0, "w": w1, "b": b1, "beta": bn1[1]}

    def run(x, w0, w, b, beta):
        with L._precision(H, precision):
            return H.conv3x3_c3_fused(x, w0, b0, bn0, w, b, [bn1[0], beta, bn1[2], bn1[3]])

    def ref(x, w0, w, b, beta):
        mid = _ref_conv(x, w0, b0, bn0, 1, False)
        return _ref_conv(mid, w, b, [bn1[0], beta, bn1[2], bn1[3]], 1, True)

    sites = [(s, "x", i, 1) for s, i in _x_sites(x)] + [("weight0", "w0", (5, 1, 1, 1), None)] + _param_sites((1, 16, 1, 1), 32)
    _sweep(f"c3_fused {h}x{w} prec{precision}", _forms(l, run, variants=(0,)), ref, args, sites, exact=precision == 0,
           nan_ok=lambda label, idx, shape: _c3_pad_tap(label, idx, shape, 2, 1))


# ------------------------------------------------------------------------------------- transposed convolution, 1x1
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("cin,cout,h,w", [(64, 32, 3, 5), (128, 64, 4, 4)])
def test_convt2x2(cin, cout, h, w, precision):
    """vad_convt2x2 with ReLU: vad_act in convt_pkernel.h's epilogue (every decoder block ends here), default and one-CU plan."""
    import hip_helpers as H
    l = H.hip.lib()
    rng = L._rng(cin + cout * 7 + h + 14)
    x = rng.standard_normal((3, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cin, cout, 2, 2)) * np.sqrt(1.0 / cin)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    bn = [a.astype(np.float32) for a in (rng.uniform(0.5, 1.5, cout), rng.standard_normal(cout) * 0.1,
                                         rng.standard_normal(cout) * 0.1, rng.uniform(0.25, 1.75, cout))]
    args = {"x": x, "w": wt, "b": b, "beta": bn[1]}

    def run(x, w, b, beta):
        with L._precision(H, precision):
            return H.convt2x2(x, w, b, [bn[0], beta, bn[2], bn[3]], 2)

    ref = lambda x, w, b, beta: _ref_convt(x, w, b, [bn[0], beta, bn[2], bn[3]], 2)
    sites = [(s, "x", i, 1) for s, i in _x_sites(x)] + _param_sites((cin // 2, 1, 0, 1), cout)
    _sweep(f"convt {cin}->{cout} {h}x{w} prec{precision}", _forms(l, run, variants=()), ref, args, sites, exact=precision == 0)


def test_conv1x1():
    """vad_conv1x1 (64 -> 32, no activation): the projection in front of the decoder must hand a NaN on."""
    import hip_helpers as H
    rng = L._rng(96 + 15)
    x = rng.standard_normal((3, 64, 5, 7)).astype(np.float32)
    wt = (rng.standard_normal((32, 64, 1, 1)) * np.sqrt(1.0 / 64)).astype(np.float32)
    b = (rng.standard_normal(32) * 0.1).astype(np.float32)
    ref = lambda x, w, b: _ref_conv(x, w, b, None, 0, False, pad=0)
    sites = [(s, "x", i, 1) for s, i in _x_sites(x)] + _param_sites((1, 32, 0, 0), 32, bn=False)
    run = lambda x, w, b: H.conv1x1(x, w, b)
    _sweep("conv1x1", _forms(H.hip.lib(), run, variants=()), ref, {"x": x, "w": wt, "b": b}, sites, exact=True)


# ------------------------------------------------------------------------------------------------ fused decoder tail
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("n,h,w", [(2, 8, 24), (1, 5, 72)])
def test_dec4_tail(n, h, w, fused):
    """dec4.0 (convT + BN + ReLU) + dec4.3 (conv 32->3 + tanh) + squared error + frame score, as the fused kernel
    (dec4_fused.hip: its ReLU between the two GEMMs was an integer max with 0, which turned a NaN with the sign bit set into 0)
    and as the two launches it replaces (convt_pkernel.h's vad_act, tail.hip).  The reconstruction footprint, the error-map
    footprint and the frame's score are NaN for BOTH NaN signs; the other frame (n = 2) keeps every bit.  tanh(+-Inf) = +-1 is
    finite: there the kernels must give the reference's value."""
    import hip_helpers as H
    case = L._dec4_case(L._rng(n * 1000 + h * 10 + w + 16), n, h, w)
    x_in, wt, bt, bn, w3, b3, frames = case
    f = n - 1

    def ref(x, wt, w3):
        act = torch.relu(_bn64(F.conv_transpose2d(_t64(x), _t64(wt), _t64(bt), stride=2), bn))
        recon = torch.tanh(F.conv2d(act, _t64(w3), _t64(b3), padding=1))
        emap = ((_t64(frames) - recon) ** 2).mean(dim=1)
        return recon.numpy(), emap.numpy(), emap.mean(dim=(1, 2)).numpy()

    def run(x, wt, w3):
        return L._dec4_run(H, (x, wt, bt, bn, w3, b3, frames), fused=fused)

    sites = [("x-interior", "x", (f, 16, _odd(h), _odd(w)), f), ("x-last", "x", (f, 31, h - 1, w - 1), f),
             ("convt-weight", "wt", (5, 7, 1, 0), None), ("conv-weight", "w3", (1, 9, 1, 1), None)]
    ref_c, got_c = ref(x_in, wt, w3), run(x_in, wt, w3)
    assert np.isfinite(got_c[2]).all()
    for label, key, idx, frame in sites:
        args = {"x": x_in, "wt": wt, "w3": w3}
        ref_nan = ref(**{**args, key: _put(args[key], idx, "+nan")})
        for poison in POISONS:
            tag = f"dec4 fused={fused} {label} {poison}"
            pa = {**args, key: _put(args[key], idx, poison)}
            ref_p, got_p = ref(**pa), run(**pa)
            for o in range(2):                                                    # recon, error map
                fr = frame if n > 1 else None
                if fr is None:                                                    # (no second frame: only the in-frame masks)
                    assert not (frame is not None and (~(ref_p[o] == ref_c[o])).all()), tag
                nk = None
                if not fused:                                 # vad_conv3x3_to3_score's padding by 0 (module docstring): the border
                    nk = np.zeros(ref_p[o].shape, bool)
                    nk[..., [0, -1], :] = True
                    nk[..., :, [0, -1]] = True
                    nk &= np.isnan(ref_nan[o])
                _check(f"{tag} out{o}", poison, got_c[o], got_p[o], ref_c[o], ref_p[o], ref_nan[o], True, ATOL, None, fr, nk)
            for i in range(n):                                                    # scores
                if frame is not None and i != frame:
                    assert _bits_equal(got_p[2][i:i + 1], got_c[2][i:i + 1]), tag
                elif not np.isfinite(ref_p[2][i]):
                    assert not np.isfinite(got_p[2][i]) and (np.isnan(got_p[2][i]) or not np.isnan(ref_p[2][i])), tag
                elif fused or np.isfinite(got_p[2][i]):       # (two launches: a border NaN of the error map may reach the score)
                    assert abs(got_p[2][i] - ref_p[2][i]) < 1e-5 * ref_p[2][i], tag
            if poison in NANS:
                assert np.isnan(ref_p[2][f]) and np.isnan(got_p[2][f]), tag


# ---------------------------------------------------------------------------------------------------------- ConvLSTM
def _ref_lstm(x, h, c, w, b):
    st = {"c.conv.weight": _t64(w), "c.conv.bias": _t64(b)}
    h2, c2 = torch_oracle.convlstm_cell(st, "c", _t64(x), _t64(h), _t64(c))
    return h2.numpy(), c2.numpy()


@pytest.mark.parametrize("cx,hid,h,w", [(64, 64, 5, 9), (32, 64, 3, 4)])
def test_convlstm_step(cx, hid, h, w):
    """vad_convlstm_step in every exact-fp32 form (the cost model's pick; 1|64: the four-gates-per-wave small-grid kernel; 1|128:
    the gate-split kernel, whose gates meet through LDS; 1|8: the persistent 32x32x2 kernel; 0: one tile per work-group; the
    one-CU plan), x, h_prev, c_prev and one gate weight poisoned in turn, masks applied to h_out AND c_out.  c is pointwise: its
    footprint is one element.  sigmoid / tanh saturate at +-Inf, so most Inf cases are finite in the reference and must match."""
    import hip_helpers as H
    x, hp, cp, wt, b = L._lstm_case(L._rng(cx + hid + h + 17), 3, cx, hid, h, w)
    args = {"x": x, "h": hp, "c": cp, "w": wt}
    run = lambda x, h, c, w: H.convlstm_step(x, h, c, w, b)
    ref = lambda x, h, c, w: _ref_lstm(x, h, c, w, b)
    pos = (1, 5, _odd(h), _odd(w))
    sites = [("x-interior", "x", pos, 1), ("x-last", "x", (1, cx - 1, h - 1, w - 1), 1), ("h-interior", "h", pos, 1),
             ("c-interior", "c", pos, 1), ("gate-weight", "w", (hid + 3, cx // 2, 1, 1), None)]
    _sweep(f"convlstm {cx}/{hid} {h}x{w}", _forms(H.hip.lib(), run, variants=(1 | 64, 1 | 128, 1 | 8, 0)), ref, args, sites, exact=True,
           atol=LSTM_ATOL, outputs=2)


@pytest.mark.parametrize("precision", ["split", "wino"])
def test_convlstm_step_split_and_wino(precision):
    """The split-fp16 step and vad_convlstm_step_wino at (64, 64, 5, 9) - both need cin_x == hid, so (32, 64, 3, 4) has no such
    form.  Winograd: the x / h footprints widened to the tiles that hold the element (c is never transformed)."""
    import hip_helpers as H
    cx = hid = 64
    h, w = 5, 9
    x, hp, cp, wt, b = L._lstm_case(L._rng(cx + hid + h + 18), 3, cx, hid, h, w)
    args = {"x": x, "h": hp, "c": cp, "w": wt}

    def run(x, h, c, w):
        if precision == "wino":
            return H.convlstm_step_wino(x, h, c, w, b)
        with L._precision(H, 1):
            return H.convlstm_step(x, h, c, w, b)

    ref = lambda x, h, c, w: _ref_lstm(x, h, c, w, b)
    pos = (1, 5, 3, 3)
    sites = [("x-interior", "x", pos, 1), ("x-last", "x", (1, cx - 1, h - 1, w - 1), 1), ("x-h-interior", "h", pos, 1),
             ("c-interior", "c", pos, 1), ("gate-weight", "w", (hid + 3, cx // 2, 1, 1), None)]
    widen = (lambda label, idx, shape: _wino_widen(label, idx, shape, False)) if precision == "wino" else None
    _sweep(f"convlstm {precision}", _forms(H.hip.lib(), run, variants=()), ref, args, sites, exact=False, atol=LSTM_ATOL, widen=widen, outputs=2)


# ------------------------------------------------------------------------------------------------------ scoring tails
def test_video_tail_and_finalize():
    """vad_convt2x2_to3_score + vad_score_finalize on 2 clips of 2 frames: a NaN in frame 2's decoder map makes that frame's
    reconstruction / error-map footprint, some of its partial sums, its score and ITS clip's sequence score NaN; the other clip
    and the clip's other frame keep every bit."""
    import hip_helpers as H
    rng = L._rng(19)
    n, h, w, t = 4, 6, 10, 2
    x_in = np.maximum(rng.standard_normal((n, 32, h, w)), 0).astype(np.float32)
    wt = (rng.standard_normal((32, 3, 2, 2)) * np.sqrt(1.0 / 32)).astype(np.float32)
    bt = (rng.standard_normal(3) * 0.1).astype(np.float32)
    frames = rng.uniform(-1, 1, (n, 3, 2 * h, 2 * w)).astype(np.float32)

    def run(x):
        recon, emap, parts = H.convt2x2_to3_score(x, wt, bt, frames)
        fs, sq = H.score_finalize(parts.reshape(n, -1), 2 * h, 2 * w, t)
        return recon, emap, parts, fs, sq

    def ref(x):
        recon = torch.tanh(F.conv_transpose2d(_t64(x), _t64(wt), _t64(bt), stride=2))
        emap = ((_t64(frames) - recon) ** 2).mean(dim=1)
        return recon.numpy(), emap.numpy()

    clean, ref_c = run(x_in), ref(x_in)
    idx = (2, 7, 3, 3)
    ref_nan = ref(_put(x_in, idx, "+nan"))
    for poison in POISONS:
        xp = _put(x_in, idx, poison)
        got, ref_p = run(xp), ref(xp)
        for o in range(2):
            _check(f"video tail {poison} out{o}", poison, clean[o], got[o], ref_c[o], ref_p[o], ref_nan[o], True, ATOL, None, 2)
        for o in (2, 3):
            assert _bits_equal(got[o][[0, 1, 3]], clean[o][[0, 1, 3]]), poison
        assert _bits_equal(got[4][:1], clean[4][:1]), poison
        if poison in NANS:
            assert np.isnan(got[2][2]).any() and np.isnan(got[3][2]) and np.isnan(got[4][1]), poison
        else:                                                  # tanh(+-Inf) = +-1: finite scores, the reference's
            want = ref_p[1][2].mean()
            assert abs(got[3][2] - want) < 1e-5 * want and np.isfinite(got[4][1]), poison


# --------------------------------------------------------------------------------------------------- training forward
@pytest.mark.parametrize("io16,wide", [(0, 1), (1, 1), (1, 0)], ids=["fp32", "bf16-wide", "bf16-narrow"])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("n,h,w,c", [(3, 8, 12, 32), (2, 6, 6, 64)])
def test_bn_act_pool_fwd(vad, n, h, w, c, act, pool, io16, wide):
    """Train-mode BatchNorm + activation + pooling (train_ops.hip: vad_act and the pooling maxima of the four- and the
    eight-channel kernel) on fp32 and bf16 tensors.  One poisoned input element makes the batch statistics of its channel, and
    with them the whole channel, NaN (Inf: mean = Inf, x - mean = NaN for every finite x, as in torch); a poisoned gamma or beta
    does the same (Inf: wherever the float64 reference is non-finite).  Every other channel keeps every bit.
    gamma = +-Inf is held to the UNFOLDED float64 composition ((y - mean) / sqrt(var + eps)) * gamma + beta, which is what the
    kernels evaluate: +-Inf by the sign of xhat, and ReLU(-Inf) = 0.  torch's fused batch_norm folds the channel into
    y * (gamma * invstd) + (beta - mean * gamma * invstd) and so forms Inf - Inf = NaN wherever y and the channel mean have the
    same sign - an artefact of that factoring, not of BatchNorm, which the kernels do not imitate (measured on MI355X against the
    fused form: 57 / 6 / 39 / 1 elements of the ReLU cases are 0 where it gives NaN)."""
    import hip_helpers as H
    l, rng = vad.hip.lib(), L._rng(n * 100 + c + act + 20)
    y = torch.from_numpy((rng.standard_normal((n, h, w, c)) * rng.uniform(0.5, 2, (1, 1, 1, c)) + rng.standard_normal((1, 1, 1, c))).astype(np.float32))
    y = y.to(torch.bfloat16).float().numpy()                                  # bf16-representable data for both storage types
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), (rng.standard_normal(c) * 0.1).astype(np.float32)
    oh, ow = (h // 2, w // 2) if pool else (h, w)
    k = 5

    def run(y, gamma, beta):
        y32 = torch.from_numpy(y).cuda()
        # (bf16 tensors by bit pattern - the data are bf16-representable: a converting cast may canonicalise a NaN's sign)
        yd = torch.from_numpy((y.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).cuda().view(torch.bfloat16) if io16 else y32
        gd, bd = H.dev(gamma), H.dev(beta)
        stats = torch.full((2 * c,), float("nan"), device="cuda")
        ws = torch.full((max(int(l.vad_chan_ws_floats(n * h * w, c)), 1),), float("nan"), device="cuda")
        vad.hip.check(l.vad_bn_stats(y32.data_ptr(), n * h * w, c, 1e-5, 0.1, stats.data_ptr(), None, None, ws.data_ptr(), H.stream()))
        out = torch.full((n, oh, ow, c), float("nan"), dtype=torch.bfloat16 if io16 else torch.float32, device="cuda")
        l.vad_debug_set_bn_wide(wide)
        try:
            vad.hip.check(l.vad_bn_act_pool_fwd_t(yd.data_ptr(), io16, stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), 0, 0, 0, 0,
                                                  n, h, w, c, act, pool, H.stream()))
        finally:
            l.vad_debug_set_bn_wide(1)
        torch.cuda.synchronize()
        if not io16:
            return out.cpu().numpy()
        return (out.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)

    def ref(y, gamma, beta):
        z = F.batch_norm(_t64(y).permute(0, 3, 1, 2), None, None, _t64(gamma), _t64(beta), training=True, eps=1e-5)
        z = _act64(z, act)
        return (F.max_pool2d(z, 2, 2) if pool else z).permute(0, 2, 3, 1).numpy()

    def ref_unfolded(y, gamma, beta):
        t = _t64(y).permute(0, 3, 1, 2)
        mean, var = t.mean(dim=(0, 2, 3), keepdim=True), t.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        z = _act64((t - mean) / torch.sqrt(var + 1e-5) * _t64(gamma).view(1, -1, 1, 1) + _t64(beta).view(1, -1, 1, 1), act)
        return (F.max_pool2d(z, 2, 2) if pool else z).permute(0, 2, 3, 1).numpy()

    assert np.abs(ref_unfolded(y, gamma, beta) - ref(y, gamma, beta)).max() < 1e-12
    clean = run(y, gamma, beta)
    assert np.isfinite(clean).all()
    other = np.ones(c, bool)
    other[k] = False
    for key, idx in (("y", (1, _odd(h), _odd(w), k)), ("gamma", (k,)), ("beta", (k,))):
        for poison in POISONS:
            tag = f"bn_act_pool {key} {poison}"
            pa = {"y": y, "gamma": gamma, "beta": beta}
            pa[key] = _put(pa[key], idx, poison)
            got, want = run(**pa), (ref_unfolded if key == "gamma" and "inf" in poison else ref)(**pa)
            assert got.shape == want.shape
            assert _bits_equal(got[..., other], clean[..., other]), f"{tag}: another channel changed"
            assert np.isfinite(want[..., other]).all()
            nf = ~np.isfinite(want)
            assert not (nf & np.isfinite(got)).any(), f"{tag}: {int((nf & np.isfinite(got)).sum())} non-finite elements of the reference are finite"
            assert not (np.isnan(want) & ~np.isnan(got)).any(), tag
            if poison in NANS or key == "y":
                assert np.isnan(want[..., k]).all() and np.isnan(got[..., k]).all(), tag


def test_lstm_gates_fwd(vad):
    """vad_lstm_gates_fwd at (1, 4, 64): one poisoned gate pre-activation (each gate in turn) or cell state reaches exactly its
    own cell - c_out and h_out of that (pixel, channel) - and every other element keeps its bits.  NaN: the cell is NaN
    (h through tanh(c)); Inf: sigmoid / tanh saturate, the float64 cell is finite except 0 * Inf forms, and the kernel follows it
    (non-finite where it is, within 1e-5 where it is finite)."""
    import hip_helpers as H
    l, rng = vad.hip.lib(), L._rng(21)
    nb, hw, hid = 1, 4, 64
    z = (rng.standard_normal((nb * hw, 4 * hid)) * 1.5).astype(np.float32)
    cp = rng.standard_normal((nb * hw, hid)).astype(np.float32)

    def run(z, cp):
        zd, cpd = H.dev(z), H.dev(cp)
        c_out, h1 = torch.full((nb * hw, hid), float("nan"), device="cuda"), torch.full((nb, hw, hid), float("nan"), device="cuda")
        h2 = torch.zeros(nb, hw, hid + 32, device="cuda")                         # the second, strided destination
        vad.hip.check(l.vad_lstm_gates_fwd(zd.data_ptr(), cpd.data_ptr(), c_out.data_ptr(), h1.data_ptr(), 0, 0,
                                           h2.data_ptr() + 4 * 32, 0, hid + 32, nb, hw, hid, H.stream()))
        torch.cuda.synchronize()
        assert H.same_bits(h2[..., 32:], h1) and float(h2[..., :32].abs().max()) == 0.0
        return c_out.cpu().numpy(), h1.cpu().numpy().reshape(nb * hw, hid)

    def ref(z, cp):
        i, f, g, o = torch.split(_t64(z), hid, dim=1)
        cn = torch.sigmoid(f) * _t64(cp) + torch.sigmoid(i) * torch.tanh(g)
        return cn.numpy(), (torch.sigmoid(o) * torch.tanh(cn)).numpy()

    clean = run(z, cp)
    assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
    pix, ch = 2, 37
    cell = np.zeros((nb * hw, hid), bool)
    cell[pix, ch] = True
    for key, idx in [("z", (pix, g * hid + ch)) for g in range(4)] + [("cp", (pix, ch))]:
        for poison in POISONS:
            pa = {"z": z, "cp": cp}
            pa[key] = _put(pa[key], idx, poison)
            got, want = run(**pa), ref(**pa)
            for o in range(2):
                tag = f"lstm_gates {key}{idx} {poison} out{o}"
                assert _bits_equal(got[o], clean[o], ~cell), tag
                if o == 1 or idx[1] < 3 * hid or key == "cp":                    # (the output gate does not reach c)
                    if poison in NANS:
                        assert np.isnan(want[o][pix, ch]) and np.isnan(got[o][pix, ch]), tag
                    elif np.isfinite(want[o][pix, ch]):
                        assert abs(got[o][pix, ch] - want[o][pix, ch]) < 1e-5, tag
                    else:
                        assert not np.isfinite(got[o][pix, ch]), tag
                else:
                    assert _bits_equal(got[o], clean[o]), tag


def test_last_layer_convt_tanh_mse(vad):
    """vad_convt_to3_mse at (2, 4, 4): a NaN in the decoder map makes the loss NaN and the reconstruction NaN on exactly its 2x2
    x 3 footprint; a NaN weight makes its output channel's parity positions and the loss NaN.  Everything outside keeps its bits."""
    import hip_helpers as H
    l, rng = vad.hip.lib(), L._rng(22)
    n, h, w = 2, 4, 4
    a = np.maximum(rng.standard_normal((n, 32, h, w)), 0).astype(np.float32)
    x = rng.uniform(-1, 1, (n, 3, 2 * h, 2 * w)).astype(np.float32)
    wt = (rng.standard_normal((32, 3, 2, 2)) / np.sqrt(32)).astype(np.float32)
    b = (rng.standard_normal(3) * 0.1).astype(np.float32)

    def run(a, wt):
        ad, wd, bd, xd = H.nhwc(a), H.dev(wt), H.dev(b), H.dev(x)
        recon = torch.full((n, 3, 2 * h, 2 * w), float("nan"), device="cuda")
        din, dpre = torch.full((n, h, w, 32), float("nan"), device="cuda"), torch.full((n * h * w, 32), float("nan"), device="cuda")
        lossd, db = torch.full((1,), float("nan"), device="cuda"), torch.full((3,), float("nan"), device="cuda")
        ws = torch.full((max(int(l.vad_convt_to3_mse_ws_floats(n, h, w)), 1),), float("nan"), device="cuda")
        vad.hip.check(l.vad_convt_to3_mse(ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), xd.data_ptr(), recon.data_ptr(), din.data_ptr(),
                                          dpre.data_ptr(), lossd.data_ptr(), db.data_ptr(), ws.data_ptr(), n, h, w, H.stream()))
        torch.cuda.synchronize()
        return recon.cpu().numpy(), float(lossd[0])

    def ref(a, wt):
        rec = torch.tanh(F.conv_transpose2d(_t64(a), _t64(wt), _t64(b), stride=2))
        return rec.numpy(), float(F.mse_loss(rec, _t64(x)))

    clean, ref_c = run(a, wt), ref(a, wt)
    assert np.isfinite(clean[1]) and abs(clean[1] - ref_c[1]) < 1e-6 * ref_c[1]
    for key, idx, frame in (("a", (1, 5, 1, 1), 1), ("wt", (5, 1, 0, 1), None)):
        ref_nan = ref(**{"a": a, "wt": wt, key: _put({"a": a, "wt": wt}[key], idx, "+nan")})
        for poison in POISONS:
            pa = {"a": a, "wt": wt}
            pa[key] = _put(pa[key], idx, poison)
            got, want = run(**pa), ref(**pa)
            _check(f"convt_to3_mse {key} {poison}", poison, clean[0], got[0], ref_c[0], want[0], ref_nan[0], True, ATOL, None, frame)
            if poison in NANS:
                assert np.isnan(want[1]) and np.isnan(got[1]), (key, poison)
            elif np.isfinite(want[1]):                                           # tanh(+-Inf) = +-1: a finite loss, the reference's
                assert abs(got[1] - want[1]) < 1e-5 * want[1], (key, poison)
            else:
                assert not np.isfinite(got[1]), (key, poison)


# -------------------------------------------------------------------------------------------------------- SSIM scoring
@pytest.mark.parametrize("window", [3, 11])
def test_ssim_score(vad, window):
    """vad_ssim_score at 32x48: a NaN pixel in frame 1 of the reconstruction (or of the target) makes the SSIM map NaN on exactly
    the window footprint the float64 composition gives, and that frame's SSIM and combined scores NaN; the map outside the
    footprint and the other frames keep every bit."""
    import hip_helpers as H
    import test_hip_ssim_score as S
    from ssim_score_ref import ssim_frames
    p, t = S._pair(23, 3, 3, 32, 48)
    mse = H.dev(((p - t) ** 2).mean(axis=(1, 2, 3)))

    def run(p, t):
        out = S._kernel(vad, H.dev(p), H.dev(t), window, 0.5, mse)
        return {k: v.cpu().numpy() for k, v in out.items()}

    clean = run(p, t)
    assert all(np.isfinite(v).all() for v in clean.values())
    for key, idx in (("p", (1, 1, 13, 21)), ("t", (1, 2, 31, 0))):
        for poison in NANS:
            pa = {"p": p, "t": t}
            pa[key] = _put(pa[key], idx, poison)
            got = run(**pa)
            _, ref_map = ssim_frames(pa["p"], pa["t"], window)
            foot = np.isnan(ref_map.numpy())
            half = window // 2
            assert foot[1].any() and not foot[1].all() and not foot[[0, 2]].any()
            assert foot.sum() == (min(31, idx[2] + half) - max(0, idx[2] - half) + 1) * (min(47, idx[3] + half) - max(0, idx[3] - half) + 1)
            assert np.array_equal(np.isnan(got["ssim_map"]), foot), (key, poison)
            assert _bits_equal(got["ssim_map"], clean["ssim_map"], ~foot), (key, poison)
            for k in ("ssim", "combined"):
                assert np.isnan(got[k][1]) and _bits_equal(got[k][[0, 2]], clean[k][[0, 2]]), (key, poison, k)


# ------------------------------------------------------------------------------------------------------------ models
def _state_t(st, dtype=torch.float64):
    return {k: (torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v))) for k, v in st.items()}


def _load(m, st):
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in st.items()}, strict=True)


def _weight_index(a):
    """The centre tap of a 3x3 weight's element [1, 1] (no zero padding meets it); element 1 of anything else."""
    return (1, 1, 1, 1) if a.ndim == 4 and a.shape[-1] == 3 else tuple(np.unravel_index(1, a.shape))


def _np(out):
    return {k: v.float().cpu().numpy() for k, v in out.items() if torch.is_tensor(v)}


IMG_STAGES = [f"encoder.enc{i}.{j}.weight" for i in range(1, 5) for j in (0, 3)] + ["encoder.enc2.1.running_var"] + \
             [f"decoder.dec{i}.{j}.weight" for i in range(1, 5) for j in (0, 3)]


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
def test_image_model(vad, precision):
    """ConvAutoencoder (latent 64, three 32x32 frames).  A NaN / Inf pixel in frame 1: its score is non-finite as in the float64
    composition of the stock module (oracle/torch_oracle.py), frames 0 and 2 keep every bit of score, error map and
    reconstruction.  Then one poisoned weight per stage - every encoder conv, a running_var, every decoder block, the last layer
    - on float and on uint8 input: every score is non-finite wherever the stock composition's is (before the fix the decoder's
    ReLUs turned these into finite scores).  Both `vad_debug_set_dec4_fused` settings."""
    l = vad.hip.lib()
    m = vad.ConvAutoencoder(in_channels=3, latent_dim=64)
    st = load_synthetic(vad, m, 51)
    m = m.cuda().eval()
    m.precision = precision
    u8 = np.random.default_rng(52).integers(0, 256, (3, 32, 32, 3), dtype=np.uint8)
    x = np.ascontiguousarray(vad.synth.u8_to_unit(u8.transpose(0, 3, 1, 2)), dtype=np.float32)

    def score(xa):
        with torch.no_grad():
            return _np(m.score_all(torch.from_numpy(xa).cuda()))

    def ref(state, xa):
        with torch.no_grad():
            return {k: v.numpy() for k, v in torch_oracle.img_scores(_state_t(state), torch.from_numpy(xa).double()).items()}

    for fused in (1, 0):
        l.vad_debug_set_dec4_fused(fused)
        try:
            clean = score(x)
            assert np.isfinite(clean["scores"]).all()
            for poison in POISONS:
                xp = _put(x, (1, 1, 5, 7), poison)
                got, want = score(xp), ref(st, xp)
                for k in ("scores", "errmap", "recon"):
                    assert _bits_equal(got[k][[0, 2]], clean[k][[0, 2]]), (poison, fused, k)
                    assert np.isfinite(want[k][[0, 2]]).all()
                    assert not (~np.isfinite(want[k]) & np.isfinite(got[k])).any(), (poison, fused, k)
                    assert not (np.isnan(want[k]) & ~np.isnan(got[k])).any(), (poison, fused, k)
                if poison in NANS:
                    assert np.isnan(want["scores"][1]) and np.isnan(got["scores"][1]), (poison, fused)
        finally:
            l.vad_debug_set_dec4_fused(1)
    try:
        for key in IMG_STAGES:
            for poison in ("+nan", "-nan", "+inf"):
                bad = dict(st)
                bad[key] = _put(st[key], _weight_index(np.asarray(st[key])), poison)
                want = ref(bad, x)["scores"]
                assert poison == "+inf" or np.isnan(want).any(), (key, poison)         # (running_var = Inf: scale 0, finite scores)                  # the case is not vacuous
                _load(m, bad)
                with torch.no_grad():
                    for inp in (torch.from_numpy(x).cuda(), torch.from_numpy(u8).cuda()):
                        got = m.get_reconstruction_error(inp).cpu().numpy()
                        assert not (~np.isfinite(want) & np.isfinite(got)).any(), f"{key} {poison} {inp.dtype}: finite scores {got} where the stock module gives {want}"
                        assert not (np.isnan(want) & ~np.isnan(got)).any(), (key, poison)
                        both = np.isfinite(want) & np.isfinite(got)
                        assert (np.abs(got[both] - want[both]) < 1e-4 * np.abs(want[both])).all(), (key, poison)
    finally:
        _load(m, st)


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
@pytest.mark.parametrize("hid,layers", [(32, 1), (64, 2)])
def test_video_model(vad, hid, layers, precision):
    """VideoAutoencoder (latent 64; hidden 32 with the 1x1 projection / hidden 64 without; b = 2, t = 3, 32x32).  A NaN pixel in
    frame 1 of clip 1: that frame and - through the ConvLSTM state - the clip's later frame are NaN as in the reference, clip 0 and
    frame 0 of clip 1 keep every bit of score, error map and reconstruction; the clip's sequence score is NaN, clip 0's is
    unchanged.  Then one poisoned weight per stage (encoder convs, a running_var, a ConvLSTM weight, proj, decoder blocks, last
    layer), float and uint8 input."""
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=64, lstm_hidden_dim=hid, lstm_num_layers=layers)
    st = load_synthetic(vad, m, 53)
    m = m.cuda().eval()
    m.precision = precision
    u8 = np.random.default_rng(54).integers(0, 256, (2, 3, 32, 32, 3), dtype=np.uint8)
    x = np.ascontiguousarray(vad.synth.u8_to_unit(u8.transpose(0, 1, 4, 2, 3)), dtype=np.float32)

    def score(xa):
        with torch.no_grad():
            return _np(m.score_all(torch.from_numpy(xa).cuda()))

    def ref(state, xa):
        with torch.no_grad():
            return {k: v.numpy() for k, v in torch_oracle.vid_scores(_state_t(state), torch.from_numpy(xa).double(), hid, layers).items()}

    clean = score(x)
    assert np.isfinite(clean["frame"]).all()
    for poison in POISONS:
        xp = _put(x, (1, 1, 1, 5, 7), poison)
        got, want = score(xp), ref(st, xp)
        for k in ("frame", "errmap", "recon"):
            assert _bits_equal(got[k][0], clean[k][0]) and _bits_equal(got[k][1, 0], clean[k][1, 0]), (poison, k)
            assert not (~np.isfinite(want[k]) & np.isfinite(got[k])).any(), (poison, k)
            assert not (np.isnan(want[k]) & ~np.isnan(got[k])).any(), (poison, k)
        assert _bits_equal(got["seq"][:1], clean["seq"][:1]), poison
        assert np.isfinite(want["frame"][0]).all() and np.isfinite(want["frame"][1, 0])
        if poison in NANS:
            assert np.isnan(want["frame"][1, 1:]).all() and np.isnan(got["frame"][1, 1:]).all() and np.isnan(got["seq"][1]), poison
    stages = [f"encoder.encoder.{i}.weight" for i in (0, 4, 8, 12)] + ["encoder.encoder.5.running_var", "convlstm.cells.0.conv.weight"] + \
             (["proj.weight"] if "proj.weight" in st else []) + [f"decoder.decoder.{i}.weight" for i in (0, 3, 6, 9)]
    assert ("proj.weight" in st) == (hid != 64)
    try:
        for key in stages:
            for poison in ("+nan", "-nan", "+inf"):
                bad = dict(st)
                bad[key] = _put(st[key], _weight_index(np.asarray(st[key])), poison)
                want = ref(bad, x)["frame"]
                assert poison == "+inf" or np.isnan(want).any(), (key, poison)         # (running_var = Inf: scale 0, finite scores)
                _load(m, bad)
                with torch.no_grad():
                    for inp in (torch.from_numpy(x).cuda(), torch.from_numpy(u8).cuda()):
                        got = m.get_reconstruction_error(inp, per_frame=True).cpu().numpy()
                        assert not (~np.isfinite(want) & np.isfinite(got)).any(), f"{key} {poison} {inp.dtype}: finite scores {got} where the stock module gives {want}"
                        assert not (np.isnan(want) & ~np.isnan(got)).any(), (key, poison)
                        both = np.isfinite(want) & np.isfinite(got)
                        assert (np.abs(got[both] - want[both]) < 1e-4 * np.abs(want[both])).all(), (key, poison)
    finally:
        _load(m, st)


def test_video_stateful_and_dense_windows(vad):
    """`score_stateful`: a NaN pixel in frame 3 of a 6-frame stream scored in two calls of three frames - the first call keeps
    every bit, the second is NaN from its first frame on, and the carried state stays poisoned: a further clean call is still NaN.
    `score_windows` (t = 3, stride 1 over 8 frames, the bad one is frame 4): windows that do not contain it keep every bit,
    windows that do have a NaN sequence score, and their frames in front of it keep theirs."""
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=64, lstm_hidden_dim=64, lstm_num_layers=2)
    load_synthetic(vad, m, 55)
    m = m.cuda().eval()
    frames = vad.synth.frames(56, 0, 8, 3, 32, 32)
    for poison in NANS:
        with torch.no_grad():
            s = torch.from_numpy(frames[None, :6]).cuda()
            sp = torch.from_numpy(_put(frames[None, :6], (0, 3, 1, 5, 7), poison)).cuda()
            a1 = m.score_stateful(s[:, :3])
            a2 = m.score_stateful(s[:, 3:], a1["state"])
            b1 = m.score_stateful(sp[:, :3])
            b2 = m.score_stateful(sp[:, 3:], b1["state"])
            b3 = m.score_stateful(s[:, 3:], b2["state"])
            assert torch.isfinite(a1["frame"]).all() and torch.isfinite(a2["frame"]).all()
            assert torch.equal(a1["frame"], b1["frame"])
            assert torch.isnan(b2["frame"]).all() and torch.isnan(b3["frame"]).all(), poison
            fr = torch.from_numpy(frames).cuda()
            frp = torch.from_numpy(_put(frames, (4, 1, 5, 7), poison)).cuda()
            c = m.score_windows(fr, sequence_length=3, stride=1, errmap=True, recon=True)
            p = m.score_windows(frp, sequence_length=3, stride=1, errmap=True, recon=True)
        assert c["seq"].shape == (6,) and torch.isfinite(c["seq"]).all()
        for k in range(6):                                                        # window k = frames k .. k + 2
            if k + 2 < 4 or k > 4:
                for key in ("seq", "frame", "errmap", "recon"):
                    assert torch.equal(p[key][k], c[key][k]), (poison, k, key)
            else:
                first = 4 - k
                assert torch.isnan(p["seq"][k]) and torch.isnan(p["frame"][k, first:]).all(), (poison, k)
                for key in ("frame", "errmap", "recon"):
                    assert torch.equal(p[key][k, :first], c[key][k, :first]), (poison, k, key)


# ----------------------------------------------------------------------------------------------------------- trainers
def _criterion(vad, loss):
    if loss == "mse":
        return nn.MSELoss()
    return vad.SSIMLoss(window_size=11) if loss == "ssim" else vad.CombinedLoss(alpha=0.5, window_size=11)


def _trainer_case(vad, make, trainer_cls, wseed, x, precision, loss, site, poison, flatten):
    """One forward_backward on a poisoned model / batch against fp32 CPU autograd of the same module in train mode."""
    ref_m = make()
    st = load_synthetic(vad, ref_m, wseed)
    xa = x
    if site == "pixel":
        xa = _put(x, tuple(0 for _ in range(x.ndim - 3)) + (1, 5, 7), poison)
    else:
        st = dict(st)
        st[site] = _put(st[site], _weight_index(np.asarray(st[site])), poison)
        _load(ref_m, st)
    ref_m.train()
    xt = torch.from_numpy(xa)
    out = ref_m(xt)
    ref_loss = _criterion(vad, loss)(out.reshape(flatten(out)), xt.reshape(flatten(xt)))
    ref_loss.backward()
    assert not torch.isfinite(ref_loss), (site, poison)                           # the case is not vacuous
    m = make()
    _load(m, st)
    m = m.cuda().train()
    tr = trainer_cls(m, precision=precision, loss=loss)
    got_loss, _ = tr.forward_backward(torch.from_numpy(xa).cuda())
    torch.cuda.synchronize()
    assert not torch.isfinite(got_loss), f"{site} {poison} {precision} {loss}: loss {float(got_loss)} where autograd gives {float(ref_loss)}"
    grads = dict(m.named_parameters())
    for k, p in ref_m.named_parameters():
        if k.endswith(".weight") and p.dim() == 4 and not torch.isfinite(p.grad).all():
            assert not torch.isfinite(grads[k].grad).all(), f"{site} {poison} {precision} {loss}: gradient of {k} is finite, autograd's is not"


VID_TRAIN_SITES = ["encoder.encoder.4.weight", "decoder.decoder.3.weight", "convlstm.cells.0.conv.weight", "pixel"]
IMG_TRAIN_SITES = ["encoder.enc2.3.weight", "decoder.dec2.0.weight", "pixel"]


@pytest.mark.parametrize("precision,loss", [("fp32", "mse"), ("split", "mse"), ("winograd", "mse"), ("bf16", "mse"), ("bf16_operands", "mse"),
                                            ("fp32", "ssim"), ("fp32", "combined")])
def test_video_trainer(vad, precision, loss):
    """VideoTrainer.forward_backward (latent 32, one layer, b = 1, t = 2, 16x16): with a NaN in an encoder conv weight, a decoder
    convT weight, an LSTM weight or an input pixel the returned loss is non-finite whenever fp32 CPU autograd's train-mode loss
    is, and every conv / convT / LSTM weight gradient autograd reports with a non-finite entry has one (before the fix: NaN batch
    statistics -> a NaN channel -> ReLU -> 0, and a finite loss)."""
    make = lambda: vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    x = vad.synth.clips(57, 0, 1, 2, 3, 16, 16)
    for site in VID_TRAIN_SITES:
        for poison in NANS:
            _trainer_case(vad, make, vad.VideoTrainer, 58, x, precision, loss, site, poison, lambda t: (-1, *t.shape[-3:]))


@pytest.mark.parametrize("precision,loss", [("fp32", "mse"), ("split", "mse"), ("winograd", "mse"), ("bf16_operands", "mse"),
                                            ("fp32", "ssim"), ("fp32", "combined")])
def test_image_trainer(vad, precision, loss):
    """ImageTrainer.forward_backward (latent 32, two 16x16 images - the smallest frames the entry point takes), as
    test_video_trainer."""
    make = lambda: vad.ConvAutoencoder(in_channels=3, latent_dim=32)
    x = vad.synth.frames(59, 0, 2, 3, 16, 16)
    for site in IMG_TRAIN_SITES:
        for poison in NANS:
            _trainer_case(vad, make, vad.ImageTrainer, 60, x, precision, loss, site, poison, lambda t: tuple(t.shape))
