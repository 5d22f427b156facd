"""References for the finite-dynamic-range tests ("Finite dynamic range of the arithmetic modes"): data with a
bounded exponent window, function-preserving power-of-two rebalancing of a state dict, and the float64 sum of |x||w| that the
split-fp16 error bounds are stated against.  CPU only: numpy and torch."""
import numpy as np
import torch
import torch.nn.functional as F


def bounded(rng, shape, emin, emax, zeros=0.3, mant_bits=23):
    """float32 values +-m * 2^e with m uniform on the `mant_bits`-bit grid of [1, 2) and integer e uniform in [emin, emax];
    round(zeros * size) of the entries, at random positions, are exact zeros (inputs behind a ReLU).  Every non-zero magnitude
    lies in [2^emin, 2^(emax + 1)): exponent-window arguments about such data are exact, not probabilistic.
    mant_bits = 7: every value is bf16-representable."""
    assert -126 <= emin <= emax <= 126 and 0 <= mant_bits <= 23 and 0.0 <= zeros < 1.0
    size = int(np.prod(shape))
    m = 1.0 + rng.integers(0, 1 << mant_bits, size).astype(np.float64) / float(1 << mant_bits)
    e = rng.integers(emin, emax + 1, size)
    v = np.ldexp(m, e) * rng.choice([-1.0, 1.0], size)
    v[rng.permutation(size)[:int(round(zeros * size))]] = 0.0
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)                             # exact in fp32 by construction
    return out.reshape(shape)


def scaled(a, k):
    """a * 2^k in float32, which must be exact (no overflow, nothing pushed into the subnormals)."""
    a = np.asarray(a, np.float32)
    out = np.ldexp(a, k).astype(np.float32)
    assert np.array_equal(np.ldexp(out.astype(np.float64), -k), a.astype(np.float64)), f"2^{k} is not an exact scaling of this array"
    return out


# --------------------------------------------------------------------------------------------------------- rebalancing
def boundaries(state, model_kind):
    """[(BatchNorm prefix, next weight key, input-channel axis of that weight, number of leading input channels concerned)] for
    every Conv/ConvT -> BatchNorm -> (Leaky)ReLU [-> MaxPool] block that is followed by another convolution, in forward order.
    image: enc1.1 -> enc1.3 ... enc4.4 -> dec1.0 ... dec4.1 -> dec4.3 (15).  video: the three inside the encoder, the last encoder
    block into the x half of ConvLSTM layer 0's gate convolution, the three inside the decoder (7).  ConvTranspose2d weights are
    (in, out, kh, kw): their input-channel axis is 0."""
    out = []
    if model_kind == "image":
        chain = [(f"encoder.enc{i}.{j}", False) for i in range(1, 5) for j in (0, 3)]
        chain += [(f"decoder.dec{i}.{j}", j == 0) for i in range(1, 5) for j in (0, 3)]
        for (conv, _), (nxt, transposed) in zip(chain[:-1], chain[1:]):
            head, idx = conv.rsplit(".", 1)
            out.append((f"{head}.{int(idx) + 1}", nxt + ".weight", 0 if transposed else 1, None))
    elif model_kind == "video":
        for a, b in ((0, 4), (4, 8), (8, 12)):
            out.append((f"encoder.encoder.{a + 1}", f"encoder.encoder.{b}.weight", 1, None))
        latent = int(np.asarray(state["encoder.encoder.12.weight"]).shape[0])
        out.append(("encoder.encoder.13", "convlstm.cells.0.conv.weight", 1, latent))
        for a, b in ((0, 3), (3, 6), (6, 9)):
            out.append((f"decoder.decoder.{a + 1}", f"decoder.decoder.{b}.weight", 0, None))
    else:
        raise ValueError(f"model_kind must be 'image' or 'video', got {model_kind!r}")
    for bn, nxt, axis, lead in out:
        c = np.asarray(state[bn + ".weight"]).shape[0]
        assert np.asarray(state[nxt]).shape[axis] >= c if lead else np.asarray(state[nxt]).shape[axis] == c, (bn, nxt)
    return out


def _mul_pow2(a, k):
    if torch.is_tensor(a):
        return torch.ldexp(a, torch.tensor(k))
    a = np.asarray(a)
    return np.ldexp(a, k).astype(a.dtype)


def rebalance(state_dict, model_kind, shifts):
    """A state dict (same container types) that computes the same function in exact arithmetic: at boundary j the BatchNorm's
    weight and bias are multiplied by 2^shifts[j] and the next convolution's weights by 2^-shifts[j] along the input channels
    that read it; nothing else moves.  LeakyReLU, ReLU and max-pooling are positively homogeneous.  `shifts`: one integer per
    entry of `boundaries`, or {index: shift}."""
    bnd = boundaries(state_dict, model_kind)
    if isinstance(shifts, dict):
        shifts = [int(shifts.get(j, 0)) for j in range(len(bnd))]
    assert len(shifts) == len(bnd), f"{len(bnd)} boundaries, {len(shifts)} shifts"
    out = dict(state_dict)
    for (bn, nxt, axis, lead), k in zip(bnd, shifts):
        k = int(k)
        if k == 0:
            continue
        out[bn + ".weight"] = _mul_pow2(out[bn + ".weight"], k)
        out[bn + ".bias"] = _mul_pow2(out[bn + ".bias"], k)
        w = out[nxt].clone() if torch.is_tensor(out[nxt]) else np.array(out[nxt])
        sl = [slice(None)] * w.ndim
        sl[axis] = slice(0, lead)
        w[tuple(sl)] = _mul_pow2(w[tuple(sl)], -k)
        out[nxt] = w
    return out


def alternating(n, k):
    """+k, -k, +k, ... for n boundaries."""
    return [k if j % 2 == 0 else -k for j in range(n)]


# ------------------------------------------------------------------------------------------------------ sum of |x||w|
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().abs()


def absconv_bound(op, x, w):
    """float64 sum over the reduction of |x||w| per output element - what a relative error of every product adds up against.
      conv3x3  x [N,Cin,H,W], w [Cout,Cin,3,3] -> [N,Cout,H,W]      (K = 9 Cin, zero padding)
      convt2x2 x [N,Cin,H,W], w [Cin,Cout,2,2] -> [N,Cout,2H,2W]    (K = Cin)
      conv1x1  x [N,Cin,H,W], w [Cout,Cin,1,1] -> [N,Cout,H,W]      (K = Cin)
      wgrad3x3 x = activations [N,Cin,H,W], w = output gradients [N,Cout,H,W] -> [Cout,Cin,3,3]   (K = N H W)
      wgrad1x1 the same for a 1x1 layer -> [Cout,Cin,1,1]"""
    x, w = _t64(x), _t64(w)
    if op == "conv3x3":
        return F.conv2d(x, w, padding=1).numpy()
    if op == "convt2x2":
        return F.conv_transpose2d(x, w, stride=2).numpy()
    if op == "conv1x1":
        return F.conv2d(x, w).numpy()
    if op == "wgrad3x3":
        n, cin, h, wd = x.shape
        cols = F.unfold(x, 3, padding=1).view(n, cin, 9, h * wd)
        return torch.einsum("nckp,nop->ock", cols, w.reshape(n, w.shape[1], h * wd)).reshape(w.shape[1], cin, 3, 3).numpy()
    if op == "wgrad1x1":
        return torch.einsum("nchw,nohw->oc", x, w)[:, :, None, None].numpy()
    raise ValueError(op)


def split_bound(sum_abs, k, bias_abs=0.0):
    """The split-fp16 bound of DESIGN.md: (3 * 2^-22) S + (K + 2) * 2^-24 (S + |b|), S = sum |x||w| over the K products."""
    s = np.asarray(sum_abs, np.float64)
    return 3.0 * 2.0 ** -22 * s + (k + 2) * 2.0 ** -24 * (s + bias_abs)
