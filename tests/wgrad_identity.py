"""Reproducible weight-gradient runs for the bit-identity test (tests/test_hip_train_ops.py): seeded inputs, one launch through
the C ABI, sha256 of the dW buffer.  The weight-gradient path has no atomics - partial slots, then a fixed-order reduce - so a
digest recorded once (tests/golden/wgrad_digests.json, written by the library as it was before the launch plan existed)
pins kernel choice, grid, split-K and reduction order of every form.  `l` is any ctypes handle of the library with the
signatures of `hip.SIGNATURES` set, so the same code runs against an older build."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import torch

# (n, h, w, cin, ncols, taps): ragged 16- and 32-pixel groups, w <= 16, the 32-channel pixel-halves tiling, wm 1 and 2, wn 2 and 4,
# the nt == 4 form of the 1x1 layers
SHAPES = [(2, 5, 20, 32, 64, 9), (2, 6, 33, 64, 128, 9), (3, 4, 16, 128, 128, 9), (2, 5, 20, 64, 256, 1), (2, 6, 33, 32, 32, 1),
          (2, 4, 16, 128, 256, 1)]
C3_SHAPES = [(2, 16, 16), (1, 8, 272)]
FORMS = ["wave_f32", "wave_bf16", "wave_split", "split_lds", "ring", "pairs", "bf16_lds"]       # include/vad_hip.h VAD_WGRAD_*
DEFAULTS = (3, 3, 1)                                                                              # pairs, split, ring_f32


def set_switches(l, switches):
    l.vad_debug_set_wgrad_pairs(switches[0])
    l.vad_debug_set_wgrad_split(switches[1])
    l.vad_debug_set_wgrad_ring_f32(switches[2])


def key(shape, precision, form, switches):
    return "x".join(map(str, shape)) + f"/p{precision}/{FORMS[form]}/" + ",".join(map(str, switches))


def cases(l):
    """Per shape and precision, the first switch setting (defaults first) of every distinct form vad_conv_wgrad_plan reports."""
    out = []
    form, slots, items = C.c_int(), C.c_longlong(), C.c_longlong()
    every = [DEFAULTS] + [s for s in itertools.product(range(4), range(4), range(2)) if s != DEFAULTS]
    try:
        for shape, precision in itertools.product(SHAPES, range(4)):
            n, h, w, cin, ncols, taps = shape
            seen = set()
            for sw in every:
                set_switches(l, sw)
                assert l.vad_conv_wgrad_plan(precision, n, h, w, cin, ncols, taps, C.byref(form), C.byref(slots), C.byref(items)) == 0
                if form.value not in seen:
                    seen.add(form.value)
                    out.append((shape, precision, form.value, sw))
    finally:
        set_switches(l, DEFAULTS)
    return out


def _digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def wgrad_inputs(shape):
    n, h, w, cin, ncols, taps = shape
    rng = np.random.default_rng(list(shape))
    return rng.standard_normal((n, h, w, cin)).astype(np.float32), (rng.standard_normal((n, h, w, ncols)) * 0.05).astype(np.float32)


def wgrad_digest(l, shape, precision, switches, inputs=None):
    n, h, w, cin, ncols, taps = shape
    a, g = inputs or wgrad_inputs(shape)
    a, g = _dev(a, precision == 3), _dev(g, precision == 3)
    ws = _nan(int(l.vad_conv_wgrad_ws_floats(n, h, taps, cin, ncols)))
    dw = _nan(ncols * cin * taps)
    set_switches(l, switches)
    try:
        rc = l.vad_conv_wgrad(a.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, cin, ncols, taps, 0 if taps == 9 else 4,
                              precision, _stream())
    finally:
        set_switches(l, DEFAULTS)
    assert rc == 0, (rc, shape, precision, switches)
    return _digest(dw)


def c3_digests(l, n, h, w):
    """First-layer weight gradient (3 input planes, 32 output channels): plain and routed form, fp32 and bf16 gradient tensors."""
    rng = np.random.default_rng([n, h, w])
    x = _dev(rng.uniform(-1, 1, (n, 3, h, w)))
    g = rng.standard_normal((n, h, w, 32)) * 1e-3
    dout = rng.standard_normal((n, h // 2, w // 2, 32)) * 1e-3
    codes = torch.from_numpy(rng.integers(0, 8, (n * (h // 2) * (w // 2), 32), dtype=np.uint8)).cuda()
    w0, b0 = _dev(rng.standard_normal((32, 3, 3, 3)) * 0.3), _dev(rng.standard_normal(32) * 0.1)
    stats = _dev(np.concatenate([rng.standard_normal(32) * 0.1, rng.uniform(0.5, 2.0, 32)]))
    gamma, ksums = _dev(rng.uniform(0.5, 1.5, 32)), _dev(rng.standard_normal(64) * 1e-4)
    ws = _nan(int(max(l.vad_conv_c3_wgrad_ws_floats(n, h, 32), l.vad_conv_c3_wgrad_routed_ws_floats(n, h))))
    assert l.vad_conv_c3_wgrad_routed_ok(h, w, 32) == 1
    out = {}
    for io16 in (0, 1):
        gd, dd, dw = _dev(g, io16), _dev(dout, io16), _nan(32 * 27)
        assert l.vad_conv_c3_wgrad_t(x.data_ptr(), gd.data_ptr(), io16, dw.data_ptr(), ws.data_ptr(), n, h, w, 32, _stream()) == 0
        out[f"c3/{n}x{h}x{w}/plain/io16={io16}"] = _digest(dw)
        dw = _nan(32 * 27)
        assert l.vad_conv_c3_wgrad_routed(x.data_ptr(), dd.data_ptr(), io16, codes.data_ptr(), w0.data_ptr(), b0.data_ptr(), stats.data_ptr(),
                                          gamma.data_ptr(), ksums.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, w, 32, _stream()) == 0
        out[f"c3/{n}x{h}x{w}/routed/io16={io16}"] = _digest(dw)
    return out
