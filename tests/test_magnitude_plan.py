"""CPU tests of the finite-dynamic-range references (tests/magnitude_ref.py) and of the host packers' refusal of weights a
split-fp16 blob cannot hold (csrc/pack.cpp; the library loads without a GPU)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import magnitude_ref as M
from conftest import load_synthetic

SPLIT, FP32, WINO = 1, 0, 4


def _module_outputs(module, st, x):
    """The stock torch.nn composition of the module in float64 (eval mode with autograd on never takes the HIP path)."""
    module.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in st.items()}, strict=True)
    module = module.double().eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return module(torch.from_numpy(x).double()).detach()


def _models(vad):
    img = lambda: vad.ConvAutoencoder(in_channels=3, latent_dim=32)
    vid = lambda: vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=2)
    return {"image": (img, vad.synth.frames(81, 0, 2, 3, 32, 32)), "video": (vid, vad.synth.clips(82, 0, 1, 2, 3, 32, 32))}


@pytest.mark.parametrize("kind,nb", [("image", 15), ("video", 7)])
def test_rebalance_preserves_the_function(vad, kind, nb):
    """+-40 at one boundary at a time and alternating +-20 at all of them: the float64 module's output equals the base model's to
    1e-12 relative (powers of two scale exactly; what is left is the summation order of a few tap products)."""
    make, x = _models(vad)[kind]
    st = load_synthetic(vad, make(), 83)
    st64 = {k: np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v) for k, v in st.items()}
    assert len(M.boundaries(st64, kind)) == nb
    base = _module_outputs(make(), st64, x)
    assert torch.isfinite(base).all() and float(base.abs().max()) > 1e-3
    plans = [{j: s} for j in range(nb) for s in (40, -40)] + [M.alternating(nb, 20), M.alternating(nb, -20)]
    for shifts in plans:
        re = M.rebalance(st64, kind, shifts)
        moved = sorted(k for k in st64 if not np.array_equal(st64[k], re[k]))
        want = 3 * (len(shifts) if isinstance(shifts, dict) else nb)
        assert len(moved) == want, (shifts, moved)                               # BN weight, BN bias, the next weight: nothing else
        got = _module_outputs(make(), re, x)
        err = float((got - base).abs().max() / base.abs().max())
        assert err <= 1e-12, f"{kind} {shifts}: {err:.3e}"


def test_rebalance_moves_the_activations():
    """Not vacuous: the rebalanced boundary's activations are the base model's times 2^shift (video: encoder block 2)."""
    import torch.nn.functional as F
    rng = np.random.default_rng(84)
    st = {"encoder.encoder.12.weight": np.zeros((8, 4, 3, 3))}
    for i, (cin, cout) in zip((0, 4, 8, 12), ((3, 4), (4, 4), (4, 4), (4, 8))):
        st[f"encoder.encoder.{i}.weight"] = rng.standard_normal((cout, cin, 3, 3))
        for k, v in (("weight", rng.uniform(0.5, 1.5, cout)), ("bias", rng.standard_normal(cout))):
            st[f"encoder.encoder.{i + 1}.{k}"] = v
    st["convlstm.cells.0.conv.weight"] = rng.standard_normal((16, 8 + 4, 3, 3))
    for i, (cin, cout) in zip((0, 3, 6, 9), ((8, 4), (4, 4), (4, 4), (4, 3))):
        st[f"decoder.decoder.{i}.weight"] = rng.standard_normal((cin, cout, 2, 2))
        if i < 9:
            st[f"decoder.decoder.{i + 1}.weight"], st[f"decoder.decoder.{i + 1}.bias"] = rng.uniform(0.5, 1.5, cout), rng.standard_normal(cout)
    re = M.rebalance(st, "video", {3: 7})
    assert np.array_equal(re["encoder.encoder.13.weight"], st["encoder.encoder.13.weight"] * 128)
    assert np.array_equal(re["encoder.encoder.13.bias"], st["encoder.encoder.13.bias"] * 128)
    w, w2 = st["convlstm.cells.0.conv.weight"], re["convlstm.cells.0.conv.weight"]
    assert np.array_equal(w2[:, :8], w[:, :8] / 128) and np.array_equal(w2[:, 8:], w[:, 8:])       # the x half only
    x = torch.from_numpy(rng.standard_normal((1, 8, 4, 4)))
    a = F.conv2d(x, torch.from_numpy(w[:, :8]), padding=1)
    b = F.conv2d(x * 128, torch.from_numpy(w2[:, :8]), padding=1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("emin,emax,zeros,bits", [(-6, 1, 0.3, 23), (-45, -45, 0.0, 23), (10, 15, 0.5, 7), (-126, 126, 0.25, 23)])
def test_bounded_keeps_its_window(emin, emax, zeros, bits):
    rng = np.random.default_rng(85)
    v = M.bounded(rng, (7, 33, 5), emin, emax, zeros, bits)
    assert v.dtype == np.float32 and v.shape == (7, 33, 5)
    assert int((v == 0).sum()) == int(round(zeros * v.size))
    nz = np.abs(v[v != 0]).astype(np.float64)
    m, e = np.frexp(nz)                                                          # nz = m 2^e, m in [0.5, 1)
    assert e.min() - 1 >= emin and e.max() - 1 <= emax
    if emax - emin < 20:
        assert set(np.unique(e - 1)) == set(range(emin, emax + 1))               # every exponent of the window occurs
    assert (v < 0).any() and (v > 0).any()
    assert np.array_equal(np.ldexp(m, 1 + bits), np.floor(np.ldexp(m, 1 + bits)))                  # the mantissa grid
    if bits == 7:
        assert np.array_equal(torch.from_numpy(v).bfloat16().float().numpy(), v)


def test_absconv_bound_is_the_sum_of_magnitudes():
    rng = np.random.default_rng(86)
    x, g = rng.standard_normal((2, 3, 4, 5)), rng.standard_normal((2, 6, 4, 5))
    w = rng.standard_normal((6, 3, 3, 3))
    s = M.absconv_bound("conv3x3", x, w)
    xp = np.pad(np.abs(x), ((0, 0), (0, 0), (1, 1), (1, 1)))
    want = sum(np.einsum("nchw,oc->nohw", xp[:, :, dy:dy + 4, dx:dx + 5], np.abs(w[:, :, dy, dx])) for dy in range(3) for dx in range(3))
    assert np.allclose(s, want, rtol=1e-13, atol=0)
    sg = M.absconv_bound("wgrad3x3", x, g)
    wantg = np.stack([np.stack([np.einsum("nchw,nohw->oc", xp[:, :, dy:dy + 4, dx:dx + 5], np.abs(g)) for dx in range(3)], -1) for dy in range(3)], -2)
    assert sg.shape == (6, 3, 3, 3) and np.allclose(sg, wantg, rtol=1e-13, atol=0)
    wt = rng.standard_normal((3, 6, 2, 2))
    st = M.absconv_bound("convt2x2", x, wt)
    assert st.shape == (2, 6, 8, 10) and np.allclose(st[:, :, 1::2, 0::2], np.einsum("nchw,co->nohw", np.abs(x), np.abs(wt[:, :, 1, 0])), rtol=1e-13, atol=0)
    assert np.allclose(M.absconv_bound("wgrad1x1", x, g)[:, :, 0, 0], np.einsum("nchw,nohw->oc", np.abs(x), np.abs(g)), rtol=1e-13, atol=0)
    assert np.allclose(M.absconv_bound("conv1x1", x, w[:, :, :1, :1]), np.einsum("nchw,oc->nohw", np.abs(x), np.abs(w[:, :, 0, 0])), rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------------- pack refusal
def _bn(cout, scale=1.0):
    arrs = [np.full(cout, scale, np.float32), np.zeros(cout, np.float32), np.zeros(cout, np.float32), np.full(cout, 1.0 - 1e-5, np.float32)]
    return arrs, (C.c_void_p * 4)(*[a.ctypes.data for a in arrs])


def _pack_layer(l, kind, w, precision, bn=None):
    """-> (rc, message, packed floats)"""
    b = np.zeros(max(w.shape[:2]), np.float32)
    bo = np.empty_like(b)
    if kind == "conv3x3":
        cout, cin = w.shape[:2]
        out = np.zeros(l.vad_pack_conv3x3_floats(cout, cin), np.float32)
        rc = l.vad_pack_conv3x3(w.ctypes.data, b.ctypes.data, bn, cout, cin, precision, out.ctypes.data, bo.ctypes.data)
    elif kind == "wino":
        cout, cin = w.shape[:2]
        out = np.zeros(l.vad_pack_conv3x3_wino_floats(cout, cin), np.float32)
        rc = l.vad_pack_conv3x3_wino(w.ctypes.data, b.ctypes.data, bn, cout, cin, out.ctypes.data, bo.ctypes.data)
    else:
        cin, cout = w.shape[:2]
        out = np.zeros(l.vad_pack_convt2x2_floats(cin, cout), np.float32)
        rc = l.vad_pack_convt2x2(w.ctypes.data, b.ctypes.data, bn, cin, cout, precision, out.ctypes.data, bo.ctypes.data)
    return rc, l.vad_last_error().decode(), out


@pytest.mark.parametrize("kind,shape,idx", [("conv3x3", (32, 16, 3, 3), (5, 9, 1, 2)), ("convt2x2", (16, 32, 2, 2), (9, 5, 1, 0))])
def test_layer_packers_refuse_what_a_split_blob_cannot_hold(vad, kind, shape, idx):
    """|folded weight| >= 65520 rounds to Inf in fp16: VAD_ERR_ARG naming the element and the value.  65519.996 (the largest fp32
    below) rounds to 65504 and packs; a BatchNorm scale folds in before the test; exact-fp32 and Winograd blobs take any finite
    value; NaN / Inf weights are packed and propagate ("Non-finite values")."""
    l = vad.hip.lib()
    rng = np.random.default_rng(87)
    w = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    rc, _, clean = _pack_layer(l, kind, w, SPLIT)
    assert rc == 0 and np.isfinite(clean.view(np.float16).astype(np.float32)).all()
    below = np.nextafter(np.float32(65520.0), np.float32(0))
    for value, refused in ((65520.0, True), (-65520.0, True), (2.0 ** 17, True), (-3.0e38, True), (below, False), (-below, False), (65504.0, False)):
        bad = w.copy()
        bad[idx] = value
        rc, msg, out = _pack_layer(l, kind, bad, SPLIT)
        assert (rc == -1) == refused, (value, rc, msg)
        if refused:
            assert f"pack_{kind}: split precision cannot hold folded weight" in msg and "65520" in msg, msg
            assert f"{float(np.float32(value)):.9g}" in msg, msg
            a, b_, t = (idx[0], idx[1], idx[2] * 3 + idx[3]) if kind == "conv3x3" else (idx[0], idx[1], idx[2] * 2 + idx[3])
            assert (f"[cout {a}][cin {b_}][tap {t}]" if kind == "conv3x3" else f"[cin {a}][cout {b_}][tap {t}]") in msg, msg
        else:
            assert np.isfinite(out.view(np.float16).astype(np.float32)).all()
        assert _pack_layer(l, kind, bad, FP32)[0] == 0
        if kind == "conv3x3":
            assert _pack_layer(l, "wino", bad, WINO)[0] == 0
    # the FOLDED weight decides: 40000 under a BatchNorm scale of 2 is 80000; 2^17 under 0.25 is 32768
    keep, bnp = _bn(shape[0] if kind == "conv3x3" else shape[1], 2.0)
    bad = w.copy()
    bad[idx] = 40000.0
    assert _pack_layer(l, kind, bad, SPLIT)[0] == 0
    rc, msg, _ = _pack_layer(l, kind, bad, SPLIT, bnp)
    assert rc == -1 and "80000" in msg, msg
    keep, bnp = _bn(shape[0] if kind == "conv3x3" else shape[1], 0.25)
    bad[idx] = 2.0 ** 17
    assert _pack_layer(l, kind, bad, SPLIT, bnp)[0] == 0
    for value in (np.inf, -np.inf, np.nan):                                       # already non-finite: packed, propagates
        bad = w.copy()
        bad[idx] = value
        assert _pack_layer(l, kind, bad, SPLIT)[0] == 0


def _model_params(vad, module, st):
    module.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in st.items()}, strict=True)
    Scorer = type(module._hip)
    return Scorer.float_params(module)


def _img_pack(vad, st, precision, in_channels=3, latent=32):
    l = vad.hip.lib()
    params = _model_params(vad, vad.ConvAutoencoder(in_channels=in_channels, latent_dim=latent), st)
    blob = np.empty(l.vad_img_packed_floats(in_channels, latent), np.float32)
    rc = l.vad_img_pack(vad.hip.pointer_array(params), len(params), in_channels, latent, precision, blob.ctypes.data)
    return rc, l.vad_last_error().decode()


def _vid_pack(vad, st, precision, layers=2):
    l = vad.hip.lib()
    params = _model_params(vad, vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=layers), st)
    blob = np.empty(l.vad_vid_packed_floats(32, 32, layers), np.float32)
    rc = l.vad_vid_pack(vad.hip.pointer_array(params), len(params), 32, 32, layers, precision, blob.ctypes.data)
    return rc, l.vad_last_error().decode()


def test_model_packers_refuse_and_name_the_layer(vad):
    """vad_img_pack / vad_vid_pack / vad_convlstm_pack with VAD_PREC_SPLIT: one weight of 2^17 in a split-packed layer -> VAD_ERR_ARG
    with the layer's state-dict name and the value; the same state packs as exact fp32 and as Winograd.  dec4.0 and the tails are
    exact fp32 in every blob and take the value.  A rebalancing shift of +20 makes a weight side of 2^20 x O(0.1): refused too."""
    st = load_synthetic(vad, vad.ConvAutoencoder(in_channels=3, latent_dim=32), 88)
    assert _img_pack(vad, st, SPLIT)[0] == 0
    for layer in ("encoder.enc1.0", "encoder.enc1.3", "encoder.enc3.0", "encoder.enc4.3", "decoder.dec1.0", "decoder.dec2.3", "decoder.dec3.0"):
        bad = dict(st)
        w = np.array(st[layer + ".weight"])
        w[1, 2, 1, 0] = -2.0 ** 17
        bad[layer + ".weight"] = w
        bn = layer[:-1] + str(int(layer[-1]) + 1)
        co = 2 if layer.startswith("decoder") and layer.endswith(".0") else 1     # (ConvTranspose2d weights are (in, out, kh, kw))
        scale = float(np.float64(st[bn + ".weight"][co]) / np.sqrt(np.float64(st[bn + ".running_var"][co]) + 1e-5))
        rc, msg = _img_pack(vad, bad, SPLIT)
        assert rc == -1 and f"img_pack: layer {layer.split('.', 1)[1]}:" in msg, (layer, msg)
        assert f"{float(np.float32(-2.0 ** 17 * scale)):.9g}" in msg, (layer, msg)
        assert _img_pack(vad, bad, FP32)[0] == 0 and _img_pack(vad, bad, WINO)[0] == 0, layer
    for layer in ("decoder.dec4.0", "decoder.dec4.3"):                            # exact fp32 in every blob
        bad = dict(st)
        w = np.array(st[layer + ".weight"])
        w[1, 2, 1, 0] = 2.0 ** 17
        bad[layer + ".weight"] = w
        assert _img_pack(vad, bad, SPLIT)[0] == 0, layer
    nb = len(M.boundaries(st, "image"))
    for j in range(nb - 2):                                                      # (the last two boundaries feed dec4.0 and dec4.3)
        rc, msg = _img_pack(vad, M.rebalance(st, "image", {j: -20}), SPLIT)
        assert rc == -1 and "split precision cannot hold" in msg, (j, msg)
    st5 = load_synthetic(vad, vad.ConvAutoencoder(in_channels=5, latent_dim=32), 89)
    bad = dict(st5)
    w = np.array(st5["encoder.enc1.0.weight"])
    w[0, 4, 2, 2] = 1e9
    bad["encoder.enc1.0.weight"] = w
    rc, msg = _img_pack(vad, bad, SPLIT, in_channels=5)
    assert rc == -1 and "img_pack: layer enc1.0:" in msg, msg
    assert _img_pack(vad, bad, FP32, in_channels=5)[0] == 0

    stv = load_synthetic(vad, vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=2), 90)
    assert _vid_pack(vad, stv, SPLIT)[0] == 0
    for layer in ("encoder.encoder.0", "encoder.encoder.8", "convlstm.cells.0.conv", "convlstm.cells.1.conv", "decoder.decoder.0", "decoder.decoder.6"):
        bad = dict(stv)
        w = np.array(stv[layer + ".weight"])
        w[1, 2, 1, 0] = 2.0 ** 17
        bad[layer + ".weight"] = w
        rc, msg = _vid_pack(vad, bad, SPLIT)
        assert rc == -1 and f"vid_pack: layer {layer}:" in msg and "split precision cannot hold" in msg, (layer, msg)
        assert _vid_pack(vad, bad, FP32)[0] == 0 and _vid_pack(vad, bad, WINO)[0] == 0, layer
    bad = dict(stv)
    w = np.array(stv["decoder.decoder.9.weight"])
    w[1, 2, 1, 0] = 2.0 ** 17
    bad["decoder.decoder.9.weight"] = w
    assert _vid_pack(vad, bad, SPLIT)[0] == 0                                     # the tail is exact fp32 in every blob

    l = vad.hip.lib()
    rng = np.random.default_rng(91)
    cells = [(rng.standard_normal((256, 128, 3, 3)) * 0.05).astype(np.float32), np.zeros(256, np.float32)]
    hids = (C.c_int * 1)(64)
    cp, hp = C.c_int(), C.c_int()
    assert l.vad_convlstm_padded_dims(64, hids, 1, C.byref(cp), C.byref(hp)) == 0
    blob = np.empty(l.vad_convlstm_packed_floats(cp.value, hp.value, 1), np.float32)
    assert l.vad_convlstm_pack(vad.hip.pointer_array(cells), 2, 64, hids, 1, SPLIT, blob.ctypes.data) == 0
    cells[0][3, 70, 0, 0] = 70000.0
    assert l.vad_convlstm_pack(vad.hip.pointer_array(cells), 2, 64, hids, 1, SPLIT, blob.ctypes.data) == -1
    msg = l.vad_last_error().decode()
    assert "convlstm_pack: layer cells.0.conv:" in msg and "= 70000 " in msg, msg
    assert l.vad_convlstm_pack(vad.hip.pointer_array(cells), 2, 64, hids, 1, FP32, blob.ctypes.data) == 0
