"""Per-launch float64 reference of one training step of the ConvLSTM video autoencoder (csrc/train_step.hip), and the
teacher-forced audit built on it.

Every launch of the step is restated here in float64 from the kernels' own statements of their arithmetic (csrc/train_ops.hip,
csrc/wgrad.hip, the comments of csrc/train_step.hip), as a function of the launch's STORED inputs.  `program()` lists the
launches in the step's serial order; the same list serves two purposes:

  * `chain()` runs it from x and the parameters, storing each output the way the mode stores it: with no rounding this is the
    model's forward and backward (tests/test_train_audit_plan.py holds it to float64 autograd), with a bf16 mode it is a
    synthetic workspace trace;
  * `audit()` runs every launch on a GIVEN trace (what a real step left in its workspace) and compares the launch's stored
    outputs with the reference.  Each check is local - errors do not accumulate - and a failure names the launch.

Each reference function returns (v, A): the value and the same computation on absolute values.  The tolerance of an element is
derived from the storage format alone (`Check.tol`):
    fp32 storage:   2^-20 A                                       (16 x the single-rounding error 2^-24 A)
    bf16 storage:   1/2 spacing_bf16(max(|got|, |v|)) + 2^-20 A    and at most 1 % of a tensor off round_bf16(v)
vad_tanh / vad_sigmoid run on the hardware transcendental unit; csrc/vad_common.h gives their absolute error as "~1e-7" (about
2e-7 against libm).  Those are typical figures, not bounds, and a tolerance needs a bound: the evaluation is three operations of
about one ulp each on values up to 2 (exp with its argument scaling, reciprocal, fma), 3 x 2^-23 = 3.6e-7 in the worst case.  A
carries 2^-21 = 4.8e-7 per evaluation (+0.5): the next power of two above that, 2.4 x the documented typical figure and half of
the 2^-20 unit every other fp32 term is allowed.  It matters for fp32-stored values only (c, h, dz, recon in the fp32 modes).

Two elements of the tolerance go beyond the issue's list, both derived: `Out.alt` - the gate pre-activations z are stored
(bf16) between the convolution and the gate kernel and then overwritten, so where the float64 pre-activation lies within the
convolution's own 2^-20 A of a bf16 rounding boundary either neighbour is an admissible input of the gate function (`audit`
counts the elements only this admitted: `alt_used`); and `stat_outs`' term for statistics restated from a convolution's inputs.

Tensor layouts are the workspace's: activations NHWC, frames n = b*T + t; ConvLSTM buffers per (layer, step) as [B, h, w, C].
"""
import numpy as np

EPS = 1e-5
U20 = 2.0 ** -20
TRANSC = 0.5                     # A-units of one vad_tanh / vad_sigmoid evaluation (see the module docstring)
ENC_C = [3, 32, 64, 128]
DEC_C = [128, 64, 32]


#: latent, hidden, layers, B, T, H, W: the smallest shapes that reach each address path of csrc/train_step.hip
#:   T1            no h1, no dh2, no c_prev, a one-pixel ConvLSTM map
#:   proj_up       proj (hidden > latent), non-square, the B > 1 frame remap, two layers
#:   three_layers  three layers, odd 3x3 ConvLSTM maps
#:   proj_down     proj (hidden < latent)
CONFIGS = [(32, 32, 1, 1, 1, 16, 16), (32, 64, 2, 2, 3, 32, 48), (64, 64, 3, 1, 4, 48, 48), (64, 32, 1, 3, 2, 32, 32)]
IDS = ["T1", "proj_up", "three_layers", "proj_down"]


def make_case(vad, cfg, seed=90):
    """The seeded model and clips of one configuration (CPU)."""
    import torch
    from conftest import load_synthetic
    latent, hid, layers, b, t, h, w = cfg
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=layers)
    load_synthetic(vad, m, seed + latent + hid + layers)
    return m, torch.from_numpy(vad.synth.clips(seed + 100, 0, b, t, 3, h, w))


# ------------------------------------------------------------------------------------------------ number formats
def spacing_bf16(x):
    """2^(floor(log2 |x|) - 7): the distance between neighbouring bf16 values at |x| (0 at 0)."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.where(x > 0, np.ldexp(1.0, e - 8), 0.0)


def round_bf16(v):
    """float64 -> nearest bf16 (ties to even), as float64; rounded once (not through fp32)."""
    v = np.asarray(v, np.float64)
    s = spacing_bf16(v)
    return np.where(s > 0, np.round(v / np.where(s > 0, s, 1.0)) * s, 0.0)


def trunc_bf16(v):
    v = np.asarray(v, np.float64)
    s = spacing_bf16(v)
    return np.where(s > 0, np.trunc(v / np.where(s > 0, s, 1.0)) * s, 0.0)


def _ident(a):
    return a


class Mode:
    """Where a mode rounds to bf16 (nearest even) - the executable form of DESIGN.md's "Arithmetic contract of the training
    step by mode".  op3: the matrix operands of the 3x3 / transposed convolutions (forward, data gradients) and of every
    weight-gradient GEMM; op1: the first layer's operands and the 1x1 convolutions (proj forward, proj / convT data gradients);
    st: every activation / activation-gradient tensor on store."""

    def __init__(self, name):
        assert name in ("fp32", "bf16_operands", "bf16", "exact")
        self.name = name
        self.store = name == "bf16"
        self.op3 = round_bf16 if name in ("bf16", "bf16_operands") else _ident
        self.op1 = round_bf16 if name == "bf16" else _ident
        self.st = round_bf16 if self.store else _ident


# ------------------------------------------------------------------------------------------------ launch references
def _mm(a, b):
    return a @ b, np.abs(a) @ np.abs(b)


def _patches3(x):
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 2, w + 2, c))
    xp[:, 1:-1, 1:-1] = x
    return np.stack([xp[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], axis=3)      # [n,h,w,9,c]


def conv3x3_fwd(x, w, b, rnd=_ident):
    """x [n,h,w,ci], w OIHW, zero padding 1: out = b + sum taps."""
    n, h, wd, ci = x.shape
    co = w.shape[0]
    v, a = _mm(_patches3(rnd(x)).reshape(-1, 9 * ci), rnd(w).transpose(2, 3, 1, 0).reshape(9 * ci, co))
    b = np.zeros(co) if b is None else b
    return (v + b).reshape(n, h, wd, co), (a + np.abs(b)).reshape(n, h, wd, co)


def conv3x3_dgrad(g, w, rnd=_ident):
    """The same convolution with the taps rotated by 180 degrees and the channel roles swapped (no bias)."""
    return conv3x3_fwd(g, w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3), None, rnd)


def conv3x3_wgrad(x, g, rnd=_ident):
    ci, co = x.shape[-1], g.shape[-1]
    v, a = _mm(_patches3(rnd(x)).reshape(-1, 9 * ci).T, rnd(g).reshape(-1, co))
    f = lambda m: m.reshape(3, 3, ci, co).transpose(3, 2, 0, 1)
    return f(v), f(a)


def conv1x1_fwd(x, w, b, rnd=_ident):
    """w [co, ci] (OIHW with 1x1 taps)."""
    v, a = _mm(rnd(x).reshape(-1, x.shape[-1]), rnd(w).T)
    b = np.zeros(w.shape[0]) if b is None else b
    s = x.shape[:-1] + (w.shape[0],)
    return (v + b).reshape(s), (a + np.abs(b)).reshape(s)


def conv1x1_dgrad(g, w, rnd=_ident):
    return conv1x1_fwd(g, w.T, None, rnd)


def conv1x1_wgrad(x, g, rnd=_ident):
    """dW [co, ci] = sum over pixels of g[co] x[ci]."""
    return _mm(rnd(g).reshape(-1, g.shape[-1]).T, rnd(x).reshape(-1, x.shape[-1]))


def d2s(u):        # [n,h,w,4*c] (position q = dy*2+dx major) -> [n,2h,2w,c]
    n, h, w, c4 = u.shape
    return u.reshape(n, h, w, 2, 2, c4 // 4).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, c4 // 4)


def s2d(u):        # [n,2h,2w,c] -> [n,h,w,4*c]: the space-to-depth view the BatchNorm backward writes
    n, h2, w2, c = u.shape
    return u.reshape(n, h2 // 2, 2, w2 // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * c)


def _convt_mat(w):  # IOHW [ci,co,2,2] -> [ci, 4*co]
    return w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1)


def convt2x2_fwd(x, w, b, rnd=_ident):
    v, a = conv1x1_fwd(x, _convt_mat(w).T, np.tile(b, 4), rnd)
    return d2s(v), d2s(a)


def convt2x2_dgrad(du_s2d, w, rnd=_ident):
    return conv1x1_fwd(du_s2d, _convt_mat(w), None, rnd)


def convt2x2_wgrad(x, du_s2d, rnd=_ident):
    ci, co = x.shape[-1], du_s2d.shape[-1] // 4
    v, a = conv1x1_wgrad(x, du_s2d, rnd)                   # [4*co, ci]
    f = lambda m: m.reshape(2, 2, co, ci).transpose(3, 2, 0, 1)
    return f(v), f(a)


def bn_stats(v):
    """Batch statistics of the UNROUNDED convolution result: mean and 1/sqrt(biased variance + eps) per channel."""
    m = v.reshape(-1, v.shape[-1])
    return m.mean(0), 1.0 / np.sqrt(m.var(0) + EPS)


def stat_outs(key, v, a=None):
    """The `mean` / `invstd` outputs of a statistics launch on v.  `a` given: the statistics are those of a convolution restated
    from its INPUTS, while the kernels take them from their own fp32 result, which is itself only held to 2^-20 A per element.
    That error moves the mean by at most 2^-20 mean(A), and - d var = 2/M sum (y - mean) dy <= 2 std max|dy| - moves 1/std by at
    most 2^-20 max(A) std / (var + eps) of itself: a derived term added to the bounds of tests/test_hip_train_ops.py.  Without
    `a` (float64 statistics of the very tensor the launch stored) those bounds stand alone."""
    m = v.reshape(-1, v.shape[-1])
    mean, var = m.mean(0), m.var(0)
    extra_m, extra_i = 0.0, 0.0
    if a is not None:
        am = a.reshape(-1, a.shape[-1])
        extra_m, extra_i = U20 * am.mean(0), U20 * am.max(0) * np.sqrt(var) / (var + EPS)
    return [Out(key + ".mean", mean, kind="mean", aux=(float(np.sqrt(var.max())), extra_m)),
            Out(key + ".invstd", 1.0 / np.sqrt(var + EPS), kind="invstd", aux=extra_i)]


def windows(y):     # [n,h,w,c] -> [n,h/2,w/2,4,c], window scan order (0,0) (0,1) (1,0) (1,1)
    n, h, w, c = y.shape
    return y.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)


def unwindows(yw):
    n, oh, ow, _, c = yw.shape
    return yw.reshape(n, oh, ow, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * oh, 2 * ow, c)


def _act(v, act):
    return np.maximum(v, 0.2 * v) if act == "leaky" else np.maximum(v, 0.0)


def bn_values(y, mean, invstd, gamma, beta):
    """xhat, the BatchNorm output before the activation, and its A - bn_xhat / bn_value of csrc/train_ops.hip."""
    xh = (y - mean) * invstd
    return xh, xh * gamma + beta, (np.abs(y) + np.abs(mean)) * invstd * np.abs(gamma) + np.abs(beta)


def bn_act_pool_fwd(y, mean, invstd, gamma, beta, act, pool):
    _, v, a = bn_values(y, mean, invstd, gamma, beta)
    v = _act(v, act)
    if pool:            # max is 1-Lipschitz in every argument: the window's largest A bounds the error of the maximum
        return windows(v).max(3), windows(a).max(3)
    return v, a


def first_decisions(y, mean, invstd, gamma, beta, act, pool):
    """Decision bytes as bn_route takes them: bits 0-1 = first maximum in window scan order, bit 2 = value > 0."""
    _, v, _ = bn_values(y, mean, invstd, gamma, beta)
    v = _act(v, act)
    if pool:
        vw = windows(v)
        am = vw.argmax(3)
        ch = np.take_along_axis(vw, am[:, :, :, None, :], 3)[:, :, :, 0, :]
    else:
        am, ch = np.zeros(v.shape, np.int64), v
    return (am | np.where(ch > 0, 4, 0)).astype(np.uint8)


def verify_decisions(y, mean, invstd, gamma, beta, act, pool, dec):
    """Recorded decisions are verified, not trusted: the chosen element's float64 value lies within the fp32 tolerance of its
    window's maximum, and the recorded sign is the value's sign unless |value| is within that tolerance of zero.  (bf16 storage
    makes exact ties common: a "first maximum" rule of the reference's own would be wrong.)  Returns the worst ratio."""
    _, v, a = bn_values(y, mean, invstd, gamma, beta)
    v = _act(v, act)
    if pool:
        vw, aw = windows(v), windows(a)
        idx = (dec & 3).astype(np.int64)[:, :, :, None, :]
        ch, tol = np.take_along_axis(vw, idx, 3)[:, :, :, 0, :], U20 * aw.max(3)
        gap = vw.max(3) - ch
    else:
        ch, tol, gap = v, U20 * a, np.zeros_like(v)
        if (dec & 3).any():
            return np.inf
    pos = (dec & 4) > 0
    wrong = np.where(pos != (ch > 0), np.abs(ch), 0.0)
    tol = np.maximum(tol, 1e-300)
    return float(max((gap / tol).max(), (wrong / tol).max()))


def bn_act_pool_bwd(y, mean, invstd, gamma, beta, dout, dec, act, pool, to_s2d):
    """Pass A and pass B of the BatchNorm backward on the STORED y and statistics with the given decisions:
    dz = dout * act'(chosen), dbeta = sum dz, dgamma = sum dz xhat, k = sums / M (M = n h w of the conv output),
    dy = gamma invstd ((k == am) dz - k1 - xhat k2) for every window element.  Returns a dict of (v, A)."""
    xh = (y - mean) * invstd
    m = float(np.prod(y.shape[:-1]))
    pos = (dec & 4) > 0
    slope = np.where(pos, 1.0, 0.2 if act == "leaky" else 0.0)
    dz = dout * slope
    if pool:
        xw = windows(xh)
        idx = (dec & 3).astype(np.int64)[:, :, :, None, :]
        xc = np.take_along_axis(xw, idx, 3)[:, :, :, 0, :]
        hit = np.arange(4)[None, None, None, :, None] == idx
    else:
        xw, xc, hit = xh[:, :, :, None, :], xh, True
    red = tuple(range(dz.ndim - 1))
    s1, a1 = dz.sum(red), np.abs(dz).sum(red)
    s2, a2 = (dz * xc).sum(red), np.abs(dz * xc).sum(red)
    sc = gamma * invstd
    dzw = np.where(hit, dz[:, :, :, None, :], 0.0)
    dyw = sc * (dzw - s1 / m - xw * (s2 / m))
    ayw = np.abs(sc) * (np.abs(dzw) + a1 / m + np.abs(xw) * (a2 / m))
    if pool:
        dy, ay = unwindows(dyw), unwindows(ayw)
    else:
        dy, ay = dyw[:, :, :, 0, :], ayw[:, :, :, 0, :]
        if to_s2d:
            dy, ay = s2d(dy), s2d(ay)
    return {"dbeta": (s1, a1), "dgamma": (s2, a2), "k": (np.stack([s1 / m, s2 / m]), np.stack([a1 / m, a2 / m])), "dy": (dy, ay)}


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_gates(pre, apre):
    """Activated gates (i, f, g, o) of pre-activations [.., 4*hid] and their A: act' * A_pre + one transcendental."""
    hid = pre.shape[-1] // 4
    v, d = _sig(pre), None
    v[..., 2 * hid:3 * hid] = np.tanh(pre[..., 2 * hid:3 * hid])
    d = v * (1 - v)
    d[..., 2 * hid:3 * hid] = 1 - v[..., 2 * hid:3 * hid] ** 2
    return v, apre * (d + 2.0 ** -10) + TRANSC


def lstm_state(gates, c_prev):
    """lstm_gates_fwd_kernel's state update from the gate values AS STORED: c = f c_prev + i g (fp32), h = o tanh(c)."""
    hid = gates.shape[-1] // 4
    i, f, g, o = (gates[..., k * hid:(k + 1) * hid] for k in range(4))
    cp = np.zeros_like(i) if c_prev is None else c_prev
    c, ac = f * cp + i * g, np.abs(f * cp) + np.abs(i * g)
    t = np.tanh(c)
    return (c, ac), (o * t, np.abs(o) * ((1 - t * t + 2.0 ** -10) * ac + TRANSC + np.abs(t)))


def lstm_gates_bwd(gates, c, c_prev, dh1, dh2, dcn, adcn):
    """lstm_gates_bwd_kernel: dh = dh1 + dh2; dc = dc_next + dh o (1 - tanh(c)^2); dz = (di, df, dg, do); dc_prev = dc f."""
    hid = gates.shape[-1] // 4
    i, f, g, o = (gates[..., k * hid:(k + 1) * hid] for k in range(4))
    cp = np.zeros_like(i) if c_prev is None else c_prev
    dh, adh = np.zeros_like(i), np.zeros_like(i)
    for s in (dh1, dh2):
        if s is not None:
            dh, adh = dh + s, adh + np.abs(s)
    tc = np.tanh(c)
    dc = dcn + dh * o * (1 - tc * tc)
    adc = adcn + adh * np.abs(o) * (1 - tc * tc + np.abs(tc))
    dz = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
    az = np.concatenate([adc * np.abs(g * i * (1 - i)), adc * np.abs(cp * f * (1 - f)), adc * np.abs(i) * (1 - g * g),
                         adh * (np.abs(tc) + TRANSC) * np.abs(o * (1 - o))], -1)
    return (dz, az), (dc * f, adc * np.abs(f))


def _to3_mat(w):    # IOHW [32,3,2,2] -> [32, 12], column q*3 + c
    return w.transpose(0, 2, 3, 1).reshape(32, 12)


def to3_tanh_fwd(r, w, b):
    """recon NCHW [n,3,2h,2w] = tanh(convT(r) + b), fp32 arithmetic on the stored input; returns (recon, A)."""
    pre, ap = conv1x1_fwd(r, _to3_mat(w).T, np.tile(b, 4))
    rec = np.tanh(pre)
    a = ap * (1 - rec * rec + 2.0 ** -10) + TRANSC
    f = lambda m: d2s(m).transpose(0, 3, 1, 2)
    return f(rec), f(a)


def to3_tanh_bwd(rec, arec, drec, adrec, w, scale):
    """dp = scale * drecon * (1 - recon^2) per output element; din = dp . W; dpre = dp in 32 columns (12..31 zero)."""
    f = lambda m: s2d(m.transpose(0, 2, 3, 1))                      # NCHW -> [n,h,w,12], column q*3 + c
    rec, arec, drec, adrec = f(rec), f(arec), f(drec), f(adrec)
    dp = scale * drec * (1 - rec * rec)
    adp = scale * (adrec * (1 - rec * rec) + 2 * np.abs(drec * rec) * arec) + np.abs(dp)
    wm = _to3_mat(w)
    din, adin = dp @ wm.T, adp @ np.abs(wm.T)
    pad = lambda m: np.concatenate([m, np.zeros(m.shape[:-1] + (20,))], -1)
    return (din, adin), (pad(dp), pad(adp))


def to3_mse(r, w, b, x):
    """The fused last layer: recon, loss = mean (recon - x)^2, and the backward of `to3_tanh_bwd` from 2 (recon - x) / count."""
    rec, arec = to3_tanh_fwd(r, w, b)
    d = rec - x
    loss = (np.mean(d * d), np.mean(d * d + 2 * np.abs(d) * arec))
    din, dpre = to3_tanh_bwd(rec, arec, d, arec + np.abs(d), w, 2.0 / d.size)
    return (rec, arec), loss, din, dpre


def chan_sum(g):
    m = g.reshape(-1, g.shape[-1])
    return m.sum(0), np.abs(m).sum(0)


def to3_dbias(dpre):
    s, a = chan_sum(dpre)
    return s[:12].reshape(4, 3).sum(0), a[:12].reshape(4, 3).sum(0)


def c3_wgrad_routed(x, dout, dec, w0, b0, mean, invstd, gamma, k, mode):
    """The routed first-layer weight gradient (csrc/wgrad.hip, conv_c3_wgrad_routed_kernel), from x, the POOLED gradient, the
    decisions and the stored statistics / k1, k2:
        dW[co][k] = sc (T1[k][co] - k1 SX[k] - k2 invstd ((W S)[co][k] + (b - mean) SX[k])),  sc = gamma invstd,
        T1 = sum_p dz[p][co] X[p][k],  S = X^T X,  SX[k] = sum_p X[p][k],  X = the 27 taps (c*9 + tap) of pixel p.
    bf16 tensors: X, dz and W are rounded to bf16 as MFMA operands."""
    n, h, w, _ = x.shape
    rnd = mode.op1
    xp = rnd(_patches3(x).transpose(0, 1, 2, 4, 3).reshape(-1, 27))             # k = c*9 + tap
    pos = (dec & 4) > 0
    dz = rnd(dout * np.where(pos, 1.0, 0.2))
    hit = np.arange(4)[None, None, None, :, None] == (dec & 3).astype(np.int64)[:, :, :, None, :]
    dzf = unwindows(np.where(hit, dz[:, :, :, None, :], 0.0)).reshape(-1, 32)
    t1, at1 = _mm(xp.T, dzf)                                                    # [27, 32]
    s, as_ = _mm(xp.T, xp)
    sx, asx = xp.sum(0), np.abs(xp).sum(0)
    wm = rnd(w0.reshape(32, 27))
    k1, k2 = k
    ws_, aws = wm @ s, np.abs(wm) @ as_                                    # [32, 27]
    v = invstd[:, None] * (ws_ + (b0 - mean)[:, None] * sx[None, :])
    av = invstd[:, None] * (aws + (np.abs(b0) + np.abs(mean))[:, None] * asx[None, :])
    sc = (gamma * invstd)[:, None]
    dw = sc * (t1.T - k1[:, None] * sx[None, :] - k2[:, None] * v)
    adw = np.abs(sc) * (at1.T + np.abs(k1)[:, None] * asx[None, :] + np.abs(k2)[:, None] * av)
    return dw.reshape(32, 3, 3, 3), adw.reshape(32, 3, 3, 3)


# ------------------------------------------------------------------------------------------------ the program
class Out:
    """One stored output of a launch.  kind: 'act' (activation / gradient tensor: bf16 in the bf16 mode), 'f32', 'zero'
    (exactly zero), 'mean' / 'invstd' (the bounds of tests/test_hip_train_ops.py), 'dec' (decision bytes: produced by chain(),
    verified by audit()).  `alt`: a second admissible value (the other bf16 neighbour of an inner store that is a near tie)."""

    def __init__(self, key, v, a=None, kind="act", alt=None, aux=None):
        self.key, self.v, self.a, self.kind, self.alt, self.aux = key, v, a, kind, alt, aux


class Cfg:
    def __init__(self, latent, hid, layers, b, t, h, w):
        self.L, self.Hd, self.NL, self.B, self.T, self.H, self.W = latent, hid, layers, b, t, h, w
        self.N, self.h16, self.w16 = b * t, h // 16, w // 16
        self.proj = hid != latent
        self.encC = ENC_C + [latent]
        self.decC = [latent] + DEC_C

    def cx(self, l):
        return self.L if l == 0 else self.Hd


def params_from_model(model):
    """float64 parameters under the step's names (csrc/train_step.hip: e_* encoder, l_* ConvLSTM, pj_* proj, d_* decoder, t_*)."""
    sd = {k: v.detach().double().cpu().numpy() for k, v in model.named_parameters()}
    p, names = {}, {}

    def put(short, full):
        p[short], names[short] = sd[full], full
    for k in range(4):
        put(f"e_w{k}", f"encoder.encoder.{4 * k}.weight"); put(f"e_b{k}", f"encoder.encoder.{4 * k}.bias")
        put(f"e_g{k}", f"encoder.encoder.{4 * k + 1}.weight"); put(f"e_be{k}", f"encoder.encoder.{4 * k + 1}.bias")
    l = 0
    while f"convlstm.cells.{l}.conv.weight" in sd:
        put(f"l_w{l}", f"convlstm.cells.{l}.conv.weight"); put(f"l_b{l}", f"convlstm.cells.{l}.conv.bias")
        l += 1
    if "proj.weight" in sd:
        put("pj_w", "proj.weight"); put("pj_b", "proj.bias")
    for j in range(3):
        put(f"d_w{j}", f"decoder.decoder.{3 * j}.weight"); put(f"d_b{j}", f"decoder.decoder.{3 * j}.bias")
        put(f"d_g{j}", f"decoder.decoder.{3 * j + 1}.weight"); put(f"d_be{j}", f"decoder.decoder.{3 * j + 1}.bias")
    put("t_w", "decoder.decoder.9.weight"); put("t_b", "decoder.decoder.9.bias")
    return p, names


def _remap_to_slabs(v, c):      # frames b*T+t -> [T][B]
    return v.reshape((c.B, c.T) + v.shape[1:]).swapaxes(0, 1)


def _remap_to_frames(v, c):     # [T][B] -> frames b*T+t
    return v.swapaxes(0, 1).reshape((c.N,) + v.shape[2:])


def program(c, mode, P, x, routed=True):
    """The launches of one step in serial order: a list of (name, fn); fn(tr, **variant) -> [Out] reads the stored tensors of
    the trace `tr`.  `x` NCHW [N,3,H,W] float64.  `variant` keyword arguments state a defect (tests only)."""
    L, Hd, NL, B, T = c.L, c.Hd, c.NL, c.B, c.T
    xl = x.transpose(0, 2, 3, 1)
    prog = []

    def launch(name):
        def deco(fn):
            prog.append((name, fn))
            return fn
        return deco

    def cat(tr, l, t):
        return np.concatenate([tr[f"catx{l}_{t}"], tr[f"cath{l}_{t}"]], -1)

    def conv_bn(name, key, src, w, b, kind):
        @launch(name)
        def _(tr, **kw):
            if kind == "c3":
                v, a = conv3x3_fwd(xl, w, b, mode.op1)
            elif kind == "conv":
                v, a = conv3x3_fwd(tr[src], w, b, mode.op3)
            else:
                v, a = convt2x2_fwd(tr[src], w, b, mode.op3)
            return [Out(key[0], v, a)] + stat_outs(key[1], v, a)

        if not mode.store:      # fp32 tensors: y is stored unrounded, so the statistics launch can be held on its own
            @launch(name.split(".")[0] + ".stats_of_stored")
            def _(tr, **kw):
                return stat_outs(key[1], tr[key[0]])

    # ---- forward: encoder
    for k in range(4):
        conv_bn(f"enc{k}.conv_fwd", (f"y{k}", f"st_e{k}"), f"a{k - 1}", P[f"e_w{k}"], P[f"e_b{k}"], "c3" if k == 0 else "conv")

        @launch(f"enc{k}.bn_act_pool_fwd")
        def _(tr, k=k, remap=True, **kw):
            v, a = bn_act_pool_fwd(tr[f"y{k}"], tr[f"st_e{k}.mean"], tr[f"st_e{k}.invstd"], P[f"e_g{k}"], P[f"e_be{k}"], "leaky", True)
            if k < 3:
                return [Out(f"a{k}", v, a)]
            if remap:       # latent features go straight into layer 0's operand buffers: frame b*T+t -> slot t*B+b, x-part
                v, a = _remap_to_slabs(v, c), _remap_to_slabs(a, c)
            else:
                v, a = v.reshape((T, B) + v.shape[1:]), a.reshape((T, B) + a.shape[1:])
            return [Out(f"catx0_{t}", v[t], a[t]) for t in range(T)]

    # ---- forward: ConvLSTM (layers-outer order; the wavefront runs the same launches)
    @launch("lstm.zero_h0")
    def _(tr, **kw):
        z = np.zeros((B, c.h16, c.w16, Hd))
        return [Out(f"cath{l}_0", z, kind="zero") for l in range(NL)]

    for l in range(NL):
        for t in range(T):
            @launch(f"lstm_fwd[{l},{t}].gates")
            def _(tr, l=l, t=t, **kw):
                pre, ap = conv3x3_fwd(cat(tr, l, t), P[f"l_w{l}"], P[f"l_b{l}"], mode.op3)
                alt = None
                if mode.store:      # z is stored (bf16) between the convolution and the gate kernel: where the float64 value is
                    r = round_bf16(pre)   # within the convolution's own tolerance of a rounding boundary, both neighbours are admissible
                    s = spacing_bf16(pre)
                    other = np.where(pre >= r, r + s, r - s)
                    near = np.abs(np.abs(pre - r) - 0.5 * s) <= U20 * ap
                    alt = np.where(near, lstm_gates(other, np.zeros_like(ap))[0], np.nan)
                    pre, ap = r, np.zeros_like(ap)
                v, a = lstm_gates(pre, ap)
                return [Out(f"z{l}_{t}", v, a, alt=alt)]

            @launch(f"lstm_fwd[{l},{t}].state")
            def _(tr, l=l, t=t, h1_slab=None, **kw):
                (cv, ca), (h, ah) = lstm_state(tr[f"z{l}_{t}"], tr[f"c{l}_{t - 1}"] if t else None)
                outs = [Out(f"c{l}_{t}", cv, ca, kind="f32")]
                if t + 1 < T or h1_slab is not None:
                    outs.append(Out(f"cath{l}_{t + 1 if h1_slab is None else h1_slab}", h, ah))
                outs.append(Out(f"catx{l + 1}_{t}" if l + 1 < NL else f"hseq_{t}", h, ah))
                return outs

    def hseq(tr):       # [N = b*T+t, h, w, Hd]
        return _remap_to_frames(np.stack([tr[f"hseq_{t}"] for t in range(T)]), c)

    if c.proj:
        @launch("proj.fwd")
        def _(tr, **kw):
            v, a = conv1x1_fwd(hseq(tr), P["pj_w"][:, :, 0, 0], P["pj_b"], mode.op1)
            return [Out("pseq", v, a)]

    def dec_in(tr):
        return tr["pseq"] if c.proj else hseq(tr)

    # ---- forward: decoder
    for j in range(3):
        @launch(f"dec{j}.convt_fwd")
        def _(tr, j=j, **kw):
            v, a = convt2x2_fwd(dec_in(tr) if j == 0 else tr[f"r{j - 1}"], P[f"d_w{j}"], P[f"d_b{j}"], mode.op3)
            return [Out(f"u{j}", v, a)] + stat_outs(f"st_d{j}", v, a)

        if not mode.store:
            @launch(f"dec{j}.stats_of_stored")
            def _(tr, j=j, **kw):
                return stat_outs(f"st_d{j}", tr[f"u{j}"])

        @launch(f"dec{j}.bn_act_fwd")
        def _(tr, j=j, **kw):
            v, a = bn_act_pool_fwd(tr[f"u{j}"], tr[f"st_d{j}.mean"], tr[f"st_d{j}.invstd"], P[f"d_g{j}"], P[f"d_be{j}"], "relu", False)
            return [Out(f"r{j}", v, a)]

    # ---- last layer + MSE, forward and backward
    @launch("to3_mse")
    def _(tr, **kw):
        (rec, arec), loss, (din, adin), (dpre, adpre) = to3_mse(tr["r2"], P["t_w"], P["t_b"], x)
        return [Out("recon", rec, arec, kind="f32"), Out("loss", np.array(loss[0]), np.array(loss[1]), kind="f32"),
                Out("dr2", din, adin), Out("dpre", dpre, adpre)]

    @launch("to3.dbias")
    def _(tr, **kw):
        return [Out("G.t_b", *to3_dbias(tr["dpre"]), kind="f32")]

    @launch("to3.wgrad")
    def _(tr, **kw):
        v, a = conv1x1_wgrad(tr["r2"], tr["dpre"][..., :12], mode.op3)          # [12, 32], row q*3 + c
        f = lambda m: m.reshape(2, 2, 3, 32).transpose(3, 2, 0, 1)
        return [Out("G.t_w", f(v), f(a), kind="f32")]

    def bn_bwd(name, ykey, stkey, g, be, doutkey, deckey, act, pool, to_s2d, outkey, gkeys, bias_key, dout_fn=None, emit_dy=True):
        @launch(name)
        def _(tr, **kw):
            y, mean, invstd = tr[ykey], tr[stkey + ".mean"], tr[stkey + ".invstd"]
            dout = dout_fn(tr) if dout_fn else tr[doutkey]
            outs = []
            if deckey in tr:
                outs.append(Out(deckey, verify_decisions(y, mean, invstd, g, be, act, pool, tr[deckey]), kind="dec"))
                dec = tr[deckey]
            else:
                dec = first_decisions(y, mean, invstd, g, be, act, pool)
                outs.append(Out(deckey, dec, kind="dec"))
            r = bn_act_pool_bwd(y, mean, invstd, g, be, dout, dec, act, pool, to_s2d)
            outs += [Out(gkeys[0], *r["dgamma"], kind="f32"), Out(gkeys[1], *r["dbeta"], kind="f32"), Out(outkey + ".k", *r["k"], kind="f32"),
                     Out(bias_key, np.zeros_like(mean), kind="zero")]     # the bias in front of a batch-statistics BatchNorm: exactly 0
            if emit_dy:
                outs.append(Out(outkey, *r["dy"]))
            return outs

    # ---- backward: decoder
    for j in (2, 1, 0):
        bn_bwd(f"dec{j}.bn_bwd", f"u{j}", f"st_d{j}", P[f"d_g{j}"], P[f"d_be{j}"], f"dr{j}", f"dec_d{j}", "relu", False, True, f"du{j}",
               (f"G.d_g{j}", f"G.d_be{j}"), f"G.d_b{j}")

        @launch(f"dec{j}.convt_wgrad")
        def _(tr, j=j, **kw):
            return [Out(f"G.d_w{j}", *convt2x2_wgrad(dec_in(tr) if j == 0 else tr[f"r{j - 1}"], tr[f"du{j}"], mode.op3), kind="f32")]

        @launch(f"dec{j}.convt_dgrad")
        def _(tr, j=j, **kw):
            return [Out(f"dr{j - 1}" if j else "ddec_in", *convt2x2_dgrad(tr[f"du{j}"], P[f"d_w{j}"], mode.op1))]

    if c.proj:
        @launch("proj.wgrad")
        def _(tr, a_from_pseq=False, **kw):
            a_op = hseq(tr)
            if a_from_pseq:         # (defect) the proj OUTPUT buffer read with hseq's shape
                flat = np.concatenate([tr["pseq"].reshape(-1), np.zeros(a_op.size)])[:a_op.size]
                a_op = flat.reshape(a_op.shape)
            v, a = conv1x1_wgrad(a_op, tr["ddec_in"], mode.op3)
            return [Out("G.pj_w", v[:, :, None, None], a[:, :, None, None], kind="f32")]

        @launch("proj.dbias")
        def _(tr, **kw):
            return [Out("G.pj_b", *chan_sum(tr["ddec_in"]), kind="f32")]

        @launch("proj.dgrad")
        def _(tr, **kw):
            return [Out("dhseq", *conv1x1_dgrad(tr["ddec_in"], P["pj_w"][:, :, 0, 0], mode.op1))]

    def dhseq(tr, t):       # [B, h, w, Hd] of step t
        return _remap_to_slabs(tr["dhseq" if c.proj else "ddec_in"], c)[t]

    # ---- backward: ConvLSTM (layers-outer order, the order of the stop-stage runs)
    for l in range(NL - 1, -1, -1):
        for t in range(T - 1, -1, -1):
            @launch(f"lstm_bwd[{l},{t}].gates")
            def _(tr, l=l, t=t, drop_dh2=False, **kw):
                dh1 = dhseq(tr, t) if l == NL - 1 else tr[f"dcatx{l + 1}_{t}"]
                dh2 = tr[f"dcath{l}_{t + 1}"] if t + 1 < T and not drop_dh2 else None
                z0 = np.zeros((B, c.h16, c.w16, Hd))
                dcn, adcn = tr["_dc"][l] if t + 1 < T else (z0, z0)
                (dz, az), dcp = lstm_gates_bwd(tr[f"z{l}_{t}"], tr[f"c{l}_{t}"], tr[f"c{l}_{t - 1}"] if t else None, dh1, dh2, dcn, adcn)
                tr.setdefault("_dc", {})[l] = dcp       # the dc chain is fp32 and only its last value is stored: carried in float64
                outs = [Out(f"dzl{l}_{t}", dz, az)]
                if t == 0:
                    outs.append(Out(f"dc{l}", dcp[0], dcp[1], kind="f32"))
                return outs

            @launch(f"lstm_bwd[{l},{t}].conv_dgrad")
            def _(tr, l=l, t=t, roll=0, **kw):
                v, a = conv3x3_dgrad(tr[f"dzl{l}_{t}"], P[f"l_w{l}"], mode.op3)
                v, a = np.roll(v, roll, -1), np.roll(a, roll, -1)
                return [Out(f"dcatx{l}_{t}", v[..., :c.cx(l)], a[..., :c.cx(l)]), Out(f"dcath{l}_{t}", v[..., c.cx(l):], a[..., c.cx(l):])]

        @launch(f"lstm_bwd[{l}].wgrad")
        def _(tr, l=l, steps=T, **kw):
            xs = np.concatenate([cat(tr, l, t) for t in range(steps)])
            gs = np.concatenate([tr[f"dzl{l}_{t}"] for t in range(steps)])
            return [Out(f"G.l_w{l}", *conv3x3_wgrad(xs, gs, mode.op3), kind="f32")]

        @launch(f"lstm_bwd[{l}].dbias")
        def _(tr, l=l, **kw):
            return [Out(f"G.l_b{l}", *chan_sum(np.concatenate([tr[f"dzl{l}_{t}"] for t in range(T)])), kind="f32")]

    # ---- backward: encoder
    for k in (3, 2, 1, 0):
        dout_fn = (lambda tr: _remap_to_frames(np.stack([tr[f"dcatx0_{t}"] for t in range(T)]), c)) if k == 3 else None
        is_routed = routed and k == 0
        bn_bwd(f"enc{k}.bn_bwd", f"y{k}", f"st_e{k}", P[f"e_g{k}"], P[f"e_be{k}"], f"da{k}", f"dec_e{k}", "leaky", True, False, f"dy{k}",
               (f"G.e_g{k}", f"G.e_be{k}"), f"G.e_b{k}", dout_fn, emit_dy=not is_routed)
        if is_routed:
            @launch("enc0.wgrad_routed")
            def _(tr, **kw):
                v, a = c3_wgrad_routed(xl, tr["da0"], tr["dec_e0"], P["e_w0"], P["e_b0"], tr["st_e0.mean"], tr["st_e0.invstd"], P["e_g0"],
                                       tr["dy0.k"], mode)
                return [Out("G.e_w0", v, a, kind="f32")]
        elif k == 0:
            @launch("enc0.wgrad")
            def _(tr, **kw):
                return [Out("G.e_w0", *conv3x3_wgrad(xl, tr["dy0"]), kind="f32")]
        else:
            @launch(f"enc{k}.wgrad")
            def _(tr, k=k, **kw):
                return [Out(f"G.e_w{k}", *conv3x3_wgrad(tr[f"a{k - 1}"], tr[f"dy{k}"], mode.op3), kind="f32")]

            @launch(f"enc{k}.conv_dgrad")
            def _(tr, k=k, **kw):
                return [Out(f"da{k - 1}", *conv3x3_dgrad(tr[f"dy{k}"], P[f"e_w{k}"], mode.op3))]
    return prog


def criterion_program(c, mode, P):
    """The last layer of the SSIM / combined criteria as its own launches: tanh forward, then - from the STORED recon and
    drecon - the tanh backward into g0 / dpre (grad_mul 1) and the bias gradient."""
    prog = []

    def fwd(tr, **kw):
        return [Out("recon", *to3_tanh_fwd(tr["r2"], P["t_w"], P["t_b"]), kind="f32")]

    def bwd(tr, **kw):
        z = np.zeros_like(tr["recon"])
        (din, adin), (dpre, adpre) = to3_tanh_bwd(tr["recon"], z, tr["drecon"], np.abs(tr["drecon"]), P["t_w"], 1.0)
        return [Out("dr2", din, adin), Out("dpre", dpre, adpre)]

    def dbias(tr, **kw):
        return [Out("G.t_b", *to3_dbias(tr["dpre"]), kind="f32")]
    return [("to3.tanh_fwd", fwd), ("to3.tanh_bwd", bwd), ("to3.dbias", dbias)]


# ------------------------------------------------------------------------------------------------ chain and audit
def chain(prog, mode, defects=None, stale=None):
    """Run the program from nothing, storing every output as the mode stores it.  `defects`: {launch name: variant kwargs}, or
    {launch name: callable(outs) -> outs} to damage what a launch stores; `stale`: what the workspace held before the step, for
    a defect that leaves a buffer unwritten."""
    tr, defects = dict(stale or {}), defects or {}
    for name, fn in prog:
        d = defects.get(name)
        outs = fn(tr, **d) if isinstance(d, dict) else fn(tr)
        if callable(d):
            outs = d(outs)
        for o in outs:
            if o.kind == "act":
                tr[o.key] = o.aux(o.v) if callable(o.aux) else mode.st(o.v)
            elif o.kind != "dec" or not np.isscalar(o.v):
                tr[o.key] = o.v
    return tr


class Check:
    """The comparison of one stored output with its reference."""

    def __init__(self, launch, out, got, mode):
        self.launch, self.key, self.kind = launch, out.key, out.kind
        self.off_share, self.ratio, self.n, self.alt_used = 0.0, 0.0, 1, 0
        if out.kind == "dec":
            self.ratio = float(out.v)                       # verify_decisions' worst ratio
        elif out.kind == "zero":
            self.ratio = 0.0 if not np.any(got) else np.inf
        elif out.kind == "mean":                            # tests/test_hip_train_ops.py: 1e-6 max(1, |mean|, std); + stat_outs' term
            self.n = out.v.size
            self.ratio = float((np.abs(got - out.v) / (1e-6 * np.maximum(1.0, np.maximum(np.abs(out.v), out.aux[0])) + out.aux[1])).max())
        elif out.kind == "invstd":                          # ... and 2e-6 relative; + stat_outs' term
            self.n = out.v.size
            self.ratio = float((np.abs(got / out.v - 1) / (2e-6 + out.aux)).max())
        else:
            got, v, a = np.asarray(got, np.float64), np.asarray(out.v, np.float64), np.asarray(out.a, np.float64)
            assert got.shape == v.shape, (launch, out.key, got.shape, v.shape)
            self.n = v.size
            bf = out.kind == "act" and mode.store
            cands = [v] if out.alt is None else [v, np.where(np.isnan(out.alt), v, out.alt)]
            ratio, off, first = None, None, None
            for cv in cands:
                tol = U20 * a + (0.5 * spacing_bf16(np.maximum(np.abs(got), np.abs(cv))) if bf else 0.0)
                err = np.abs(got - cv)
                r = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))      # (tol == 0: only the exact value passes)
                o = got != round_bf16(cv) if bf else np.zeros(v.shape, bool)
                first = (r > 1.0) | o if first is None else first
                ratio = r if ratio is None else np.minimum(ratio, r)
                off = o if off is None else off & o
            self.alt_used = int((first & (ratio <= 1.0) & ~off).sum()) if out.alt is not None else 0     # admitted by `alt` alone
            self.ratio = float(ratio.max()) if v.size else 0.0
            self.off_share = float(off.mean()) if v.size else 0.0
        self.ok = bool(self.ratio <= 1.0 and self.off_share <= 0.01)

    def __repr__(self):
        return f"{self.launch}: {self.key} worst ratio {self.ratio:.3g}, off nearest-even {self.off_share:.2%} of {self.n}{'' if self.ok else '  <-- FAILS'}"


def audit(prog, tr, mode, only=None):
    """Every launch of `prog` on the stored tensors of `tr`: a list of Check.  A launch whose inputs or outputs the trace does not
    hold raises KeyError - the audit reaches a launch or says so.  `only`: a predicate on launch names."""
    checks = []
    for name, fn in prog:
        if only and not only(name):
            continue
        for o in fn(tr):
            if o.kind == "dec" and not np.isscalar(o.v):
                raise KeyError(f"{name}: the trace holds no decisions {o.key}")
            checks.append(Check(name, o, None if o.kind == "dec" else tr[o.key], mode))
    return checks


def failing_launches(checks):
    return sorted({ch.launch for ch in checks if not ch.ok})


def summarize(checks):
    """Per launch: the largest share of elements off the nearest-even value, the worst tolerance ratio, and how many elements
    only the second admissible value (`Out.alt`) admitted."""
    out = {}
    for ch in checks:
        s = out.setdefault(ch.launch, {"off_share": 0.0, "worst_ratio": 0.0, "alt_used": 0})
        s["off_share"], s["worst_ratio"] = max(s["off_share"], ch.off_share), max(s["worst_ratio"], ch.ratio)
        s["alt_used"] += ch.alt_used
    return out


# ------------------------------------------------------------------------------------------------ workspace layout
def workspace_layout(lib, c, loss_kind=0):
    """{name: (float offset, floats)} of every buffer the two debug layout queries report, and the workspace size in floats."""
    import ctypes as C
    out = (C.c_longlong * 96)()
    n = lib.vad_vid_train_debug_layout(c.B, c.T, c.H, c.W, c.L, c.Hd, c.NL, out, 96)
    assert n > 0, "vad_vid_train_debug_layout refused the configuration"
    a = list(out[:n])
    n2 = lib.vad_vid_train_debug_layout2(c.B, c.T, c.H, c.W, c.L, c.Hd, c.NL, loss_kind, out, 96)
    assert n2 > 0, "vad_vid_train_debug_layout2 refused the configuration"
    b = list(out[:n2])
    N, hw, NL = c.N, c.h16 * c.w16, c.NL
    ysz = [N * (c.H >> k) * (c.W >> k) * c.encC[k + 1] for k in range(4)]
    usz = [N * (c.h16 << (j + 1)) * (c.w16 << (j + 1)) * c.decC[j + 1] for j in range(3)]
    names = [(f"y{k}", ysz[k]) for k in range(4)] + [(f"a{k}", ysz[k] // 4) for k in range(3)]
    names += [(f"st_e{k}", 2 * c.encC[k + 1]) for k in range(4)]
    names += [(f"cat{l}", N * hw * (c.cx(l) + c.Hd)) for l in range(NL)] + [(f"z{l}", N * hw * 4 * c.Hd) for l in range(NL)]
    names += [(f"c{l}", N * hw * c.Hd) for l in range(NL)] + [("hseq", N * hw * c.Hd)]
    names += [(f"u{j}", usz[j]) for j in range(3)] + [(f"r{j}", usz[j]) for j in range(3)] + [(f"st_d{j}", 2 * c.decC[j + 1]) for j in range(3)]
    names += [("dpre", N * (c.H // 2) * (c.W // 2) * 32)] + [(f"g{i}", max(ysz + usz)) for i in range(3)]
    assert len(a) == len(names) + 1, (len(a), len(names))
    lay = {nm: (off, sz) for (nm, sz), off in zip(names, a)}
    names2 = [("pseq", N * hw * c.L if c.proj else 0)] + [(f"dcat{l}", N * hw * (c.cx(l) + c.Hd)) for l in range(NL)]
    names2 += [(f"dzl{l}", N * hw * 4 * c.Hd) for l in range(NL)] + [(f"dc{l}", c.B * hw * c.Hd) for l in range(NL)]
    img = N * 3 * c.H * c.W if loss_kind else 0
    names2 += [("recon", img), ("drecon", img), ("ksums", 2048)]
    assert len(b) == len(names2) + 1, (len(b), len(names2))
    lay.update({nm: (off, sz) for (nm, sz), off in zip(names2, b)})
    assert a[-1] == b[-1] or loss_kind, "the two layout queries disagree about the workspace size"
    return lay, b[-1]
