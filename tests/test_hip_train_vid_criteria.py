"""GPU parity of `VideoTrainer(loss="ssim" | "combined")`: the last layer as forward / criterion /
backward (`vad_convt_to3_tanh_fwd_t`, `vad_ssim_mse`, `vad_ssim_mse_backward`, `vad_convt_to3_tanh_bwd_t`) behind
`vad_vid_train_fwd_bwd_l`.  Same standards as tests/test_hip_train_step.py (MSE) and tests/test_hip_train_img.py (the image step's
criteria): the two new kernels alone against the fused MSE kernel and float64, float64 gradients with the kernels' branch decisions
imposed, the reference's own step (tests/golden/train_vid_criteria), the loss curve against CPU autograd, and the workspace
contract.  The float64 / CPU restatements live in tests/vid_train_criterion_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vid_train_criterion_ref as R
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

LR, WD = 1e-4, 1e-5
NAN = float("nan")


@pytest.fixture(autouse=True)
def _fixed_cpu_threads():
    """(the fp32 CPU side sums in an order that depends on the thread count: tests/test_hip_train_step.py)"""
    before = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(before)


# ------------------------------------------------------------------------------------------------ 1. the last-layer kernels alone
def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


class _Layer:
    """One ConvTranspose2d(32->3,k2,s2)+Tanh problem on the device: input r [n,h,w,32] in the storage type, weights, frames x."""

    def __init__(self, vad, n, h, w, io16):
        import hip_helpers as H
        self.vad, self.l, self.H = vad, vad.hip.lib(), H
        self.n, self.h, self.w, self.io = n, h, w, io16
        self.dt = torch.bfloat16 if io16 else torch.float32
        rng = np.random.default_rng(1000 * n + 10 * h + w + io16)
        self.r = H.dev(rng.standard_normal((n, h, w, 32))).to(self.dt)
        self.wt, self.bt = H.dev(rng.standard_normal((32, 3, 2, 2)) * 0.2), H.dev(rng.standard_normal(3) * 0.1)
        self.x = H.dev(rng.uniform(-1, 1, (n, 3, 2 * h, 2 * w)))
        self.count = n * 3 * 2 * h * 2 * w
        self.rng = rng

    def fused(self):
        l, H, n, h, w = self.l, self.H, self.n, self.h, self.w
        ws = _nan((max(l.vad_convt_to3_mse_ws_floats(n, h, w), 1),))
        rec, loss, db = _nan((n, 3, 2 * h, 2 * w)), _nan((1,)), _nan((3,))
        din, dpre = _nan((n, h, w, 32), self.dt), _nan((n * h * w, 32), self.dt)
        self.vad.hip.check(l.vad_convt_to3_mse_t(self.r.data_ptr(), self.io, self.wt.data_ptr(), self.bt.data_ptr(), self.x.data_ptr(),
                                                 rec.data_ptr(), din.data_ptr(), dpre.data_ptr(), loss.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                                 n, h, w, 1.0, H.stream()))
        return rec, din, dpre, db

    def fwd(self):
        rec = _nan((self.n, 3, 2 * self.h, 2 * self.w))
        self.vad.hip.check(self.l.vad_convt_to3_tanh_fwd_t(self.r.data_ptr(), self.io, self.wt.data_ptr(), self.bt.data_ptr(), rec.data_ptr(),
                                                           self.n, self.h, self.w, self.H.stream()))
        return rec

    def bwd(self, rec, drecon, grad_mul=1.0, expect_ok=True):
        l, n, h, w = self.l, self.n, self.h, self.w
        ws = _nan((l.vad_convt_to3_tanh_bwd_ws_floats(n, h, w),))
        din, dpre, db = _nan((n, h, w, 32), self.dt), _nan((n * h * w, 32), self.dt), _nan((3,))
        rc = l.vad_convt_to3_tanh_bwd_t(rec.data_ptr(), drecon.data_ptr(), self.wt.data_ptr(), din.data_ptr(), dpre.data_ptr(), self.io,
                                        db.data_ptr(), ws.data_ptr(), n, h, w, grad_mul, self.H.stream())
        torch.cuda.synchronize()
        if expect_ok:
            self.vad.hip.check(rc)
        return rc, din, dpre, db


def _dpre_layout(t_nchw, n, h, w):
    """[n,3,2h,2w] -> the kernels' [n*h*w][12] operand: column q*3+c, q = 2*dy+dx"""
    v = t_nchw.reshape(n, 3, h, 2, w, 2).permute(0, 2, 4, 3, 5, 1)          # n, y, x, dy, dx, c
    return v.reshape(n * h * w, 12)


@pytest.mark.parametrize("io16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,h,w", [(1, 8, 8), (3, 8, 24), (2, 24, 40)])
def test_last_layer_kernels_alone(vad, n, h, w, io16):
    """Forward: the fused kernel's reconstruction, bit for bit.  Backward: linear in d recon - with the MSE's own gradient it gives
    the fused kernel's outputs (fp32: the same summation order and one more rounding of d recon, held to 1e-6 of each tensor's
    largest entry; bf16 storage: one bf16 ulp of each value); with a random gradient the float64 backward of ConvTranspose2d + tanh
    (fp32 storage: 1e-5 of the largest entry; bf16 storage: that plus the half ulp, at most 2^-8 of the value, of the final rounding)."""
    L = _Layer(vad, n, h, w, io16)
    rec_f, din_f, dpre_f, db_f = L.fused()
    rec = L.fwd()
    torch.cuda.synchronize()
    assert torch.equal(rec, rec_f)

    # --- linearity: the MSE's gradient reproduces the fused kernel
    drecon = (rec - L.x) * np.float32(2.0 / L.count)
    _, din, dpre, db = L.bwd(rec, drecon)
    for name, got, want in (("din", din, din_f), ("dpre32", dpre, dpre_f), ("dbias3", db, db_f)):
        got, want = got.float(), want.float()
        assert bool(torch.isfinite(got).all()), name
        if io16:
            ulp = float(((got - want).abs() / (want.abs() * 2.0 ** -7 + 1e-30)).max())
            print(f"[{n},{h},{w},bf16] {name}: {ulp:.3f} bf16 ulp from the fused kernel")
            assert ulp <= 1.0 + 1e-6, f"{name}: {ulp:.3f} bf16 ulp from the fused kernel"
        else:
            err = float((got - want).abs().max()) / float(want.abs().max())
            print(f"[{n},{h},{w},fp32] {name}: {err:.2e} of the largest entry from the fused kernel")
            assert err <= 1e-6, f"{name}: {err:.3e} of the largest entry from the fused kernel"
    assert bool((dpre[:, 12:] == 0).all())

    # --- a random gradient against float64
    g = L.H.dev(L.rng.standard_normal((n, 3, 2 * h, 2 * w)))
    _, din, dpre, db = L.bwd(rec, g)
    r64 = L.r.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    rec64 = torch.tanh(F.conv_transpose2d(r64, L.wt.double().cpu(), L.bt.double().cpu(), stride=2))
    dp64 = g.double().cpu() * (1.0 - rec64.detach() ** 2)
    rec64.backward(g.double().cpu())
    want = {"din": r64.grad.permute(0, 2, 3, 1), "dpre32": _dpre_layout(dp64, n, h, w), "dbias3": dp64.sum((0, 2, 3))}
    got = {"din": din.double().cpu(), "dpre32": dpre[:, :12].double().cpu(), "dbias3": db.double().cpu()}
    for name in want:
        scale = float(want[name].abs().max())
        slack = 1e-5 * scale + (2.0 ** -8 * want[name].abs() if io16 and name != "dbias3" else 0.0)
        if io16 and name == "dbias3":         # the sum of the STORED dpre: n*h*w*4 terms, each off by at most half a bf16 ulp
            slack = 1e-5 * scale + 2.0 ** -8 * float(_dpre_layout(dp64, n, h, w).abs().sum(0).reshape(4, 3).sum(0).max())
        excess = float(((got[name] - want[name]).abs() - slack).max())
        print(f"[{n},{h},{w},{'bf16' if io16 else 'fp32'}] {name} vs float64: {float((got[name] - want[name]).abs().max()) / scale:.2e} of the largest entry")
        assert excess <= 0.0, f"{name}: {float((got[name] - want[name]).abs().max()) / scale:.3e} of the largest entry from float64"
    assert bool((dpre[:, 12:] == 0).all())

    # --- grad_mul: a power of two scales every output exactly; anything else is refused before a launch
    for k in (-3, 5):
        _, din_k, dpre_k, db_k = L.bwd(rec, g, 2.0 ** k)
        assert torch.equal(din_k.float(), din.float() * 2.0 ** k) and torch.equal(dpre_k.float(), dpre.float() * 2.0 ** k)
        assert torch.equal(db_k, db * 2.0 ** k)
    rc, din_3, dpre_3, db_3 = L.bwd(rec, g, 3.0, expect_ok=False)
    assert rc != 0 and b"power of two" in L.l.vad_last_error()
    assert bool(torch.isnan(din_3.float()).all() and torch.isnan(dpre_3.float()).all() and torch.isnan(db_3).all())


# ------------------------------------------------------------------------------------------------ 2. decision-conditioned float64
CASES = [(64, 2, 2, 3, 32, 41), (32, 2, 2, 2, (48, 80), 45), ((32, 64), 2, 2, 3, 32, 48), (32, 1, 1, 1, 16, 50)]


@pytest.mark.parametrize("latent,layers,b,t,hw,wseed", CASES)
@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
@pytest.mark.parametrize("window", [11, 7])
@pytest.mark.parametrize("loss,alpha", [("ssim", 0.5), ("combined", 0.3)])
def test_criterion_gradients_match_decision_conditioned_float64(vad, loss, alpha, window, precision, latent, layers, b, t, hw, wseed):
    """The cases are four of tests/test_hip_train_step.py's MSE list.  The criterion does not enter the forward, so the conditions on
    the decisions are that test's; loss within 5e-6 relative and every gradient within 2e-4 of its tensor's largest entry are the
    image criteria test's bounds, for the same SSIM arithmetic."""
    h, w = hw if isinstance(hw, tuple) else (hw, hw)
    x = torch.from_numpy(vad.synth.clips(wseed + 100, 0, b, t, 3, h, w))
    m = R.make(vad, latent, layers, wseed).cuda()
    tr = vad.VideoTrainer(m, lr=LR, weight_decay=WD, precision=precision, loss=loss, ssim_weight=alpha, window_size=window)
    loss_gpu, decisions = R.record_decisions(vad, tr, x.cuda())
    got = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}
    loss64, want, report = R.conditioned_float64(vad, latent, layers, wseed, x, decisions, loss, alpha, window)
    for stage, ndiff, margin, total in report:
        assert ndiff <= max(3, total // 100000), f"{stage}: {ndiff} of {total} branch decisions differ from float64"
        assert margin < 2e-4, f"{stage}: a differing decision has margin {margin:.3e}"
    print(f"[{loss},{window},{precision},{latent},{layers},{b}x{t},{hw}] loss {loss_gpu:.7f} vs float64 {loss64:.7f}: {abs(loss_gpu - loss64) / abs(loss64):.2e}")
    assert abs(loss_gpu - loss64) < 5e-6 * abs(loss64), (loss_gpu, loss64)
    zero_true, worst = R.bn_fed_biases(m), 0.0
    for k, r in want.items():
        if k in zero_true:
            assert float(np.abs(got[k]).max()) == 0.0, k                     # written as exact zeros
            continue
        assert np.isfinite(got[k]).all(), k
        worst = max(worst, float(np.abs(got[k] - r).max()) / max(float(np.abs(r).max()), 1e-12))
    print(f"[{loss},{window},{precision},{latent},{layers},{b}x{t},{hw}] worst gradient deviation {worst:.2e}; "
          f"differing decisions {[(s_, n_) for s_, n_, _, _ in report if n_]}")
    assert worst < 2e-4, f"worst gradient deviation {worst:.3e} from the decision-conditioned float64 gradient"


# ------------------------------------------------------------------------------------------------ 3. the reference's own step
@pytest.mark.parametrize("tag", ["ssim", "combined"])
def test_criterion_step_matches_reference_golden(vad, golden, tag):
    """The REFERENCE's VideoAutoencoder.train() + its SSIMLoss() / CombinedLoss(alpha=0.5) on the frames as one batch +
    torch.optim.Adam(lr 1e-4, weight_decay 1e-5), three steps on one seeded batch
    (tests/golden/train_vid_criteria/make_golden_train_vid_criteria.py).  Assertions and bounds: those of
    test_train_step_matches_reference_golden in tests/test_hip_train_step.py, exact fp32."""
    g = golden(f"train_vid_criteria/{tag}.npz")
    assert str(g["criterion"]) == tag
    latent, layers, b, t, hw, wseed, xseed, steps = (int(g[k]) for k in ("latent", "layers", "b", "t", "hw", "wseed", "xseed", "steps"))
    x = torch.from_numpy(vad.synth.clips(xseed, 0, b, t, 3, hw, hw)).cuda()
    m = R.make(vad, latent, layers, wseed)
    init = {k: v.detach().clone().numpy() for k, v in m.state_dict().items()}
    m = m.cuda()
    tr = vad.VideoTrainer(m, lr=LR, weight_decay=WD, precision="fp32", loss=tag, ssim_weight=float(g["alpha"]), window_size=int(g["window"]))
    loss0, _ = tr.forward_backward(x)
    keys = [str(k) for k in g["param_keys"]]
    got = {k: p.grad.detach().cpu().numpy().reshape(-1) for k, p in m.named_parameters()}
    assert list(got.keys()) == keys
    stride = int(g["stride"])
    zero_true = R.bn_fed_biases(m)
    for i, k in enumerate(keys):
        ref_n, ref_s = float(g["grad_norms"][i]), g[f"grad_{i}"]
        if k in zero_true:
            continue
        assert abs(float(np.linalg.norm(got[k].astype(np.float64))) - ref_n) < 3e-4 * ref_n + 1e-12, k
        scale = max(float(np.abs(ref_s).max()), 1e-12)
        assert np.abs(got[k][::stride] - ref_s).max() < 3e-4 * scale, k
    tr.optimizer_step()
    losses = [float(loss0)] + [float(tr.step(x)) for _ in range(steps - 1)]
    for a, r in zip(losses, g["losses"]):
        assert abs(a - float(r)) < 2e-5 * float(r), (losses, g["losses"])
    st = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for i, k in enumerate(str(k) for k in g["state_keys"]):
        ref = g[f"state_{i}"]
        got_s = st[k].reshape(-1)[::stride] if st[k].ndim else st[k].reshape(1)
        if k.endswith("num_batches_tracked"):
            assert int(got_s[0]) == int(ref[0]) == int(init[k]) + steps
        elif "running_" in k:
            assert np.abs(got_s - ref).max() < 1e-5 * max(1.0, np.abs(ref).max()) + 0.2 * LR * steps, k
        elif k in zero_true:
            assert np.abs(got_s - init[k].reshape(-1)[::stride]).max() <= steps * LR * 1.01
        else:
            d = np.abs(got_s - ref)
            assert np.mean(d > 0.25 * LR) < 1e-2 and d.mean() < 0.02 * LR, f"{k}: mean {d.mean():.3e}"


# ------------------------------------------------------------------------------------------------ 4. consistency
def _trainer(vad, latent=32, layers=2, wseed=55, **kw):
    return vad.VideoTrainer(R.make(vad, latent, layers, wseed).cuda(), lr=LR, weight_decay=WD, **kw)


def _clips(vad, seed=155, b=2, t=3, h=32, w=48):
    return torch.from_numpy(vad.synth.clips(seed, 0, b, t, 3, h, w)).cuda()


@pytest.mark.parametrize("loss,alpha,window", [("ssim", 0.5, 11), ("combined", 0.3, 7)])
def test_returned_loss_is_the_criterion_of_the_returned_reconstruction(vad, loss, alpha, window):
    x = _clips(vad)
    tr = _trainer(vad, loss=loss, ssim_weight=alpha, window_size=window)
    got, recon = tr.forward_backward(x, recon=True)
    crit = R.criterion(vad, loss, alpha, window)
    with torch.no_grad():
        want = float(crit(R.frames(recon), R.frames(x)))
    assert abs(float(got) - want) < 2e-6 * abs(want), (float(got), want)
    # without a caller's buffer the reconstruction lives in the workspace: the same loss and gradients, bit for bit
    grads = tr.grad.clone()
    again, none = tr.forward_backward(x)
    assert none is None and torch.equal(again, got) and torch.equal(tr.grad, grads)


def test_combined_with_weight_zero_is_the_mse_step(vad):
    x = _clips(vad)
    a, b = _trainer(vad, loss="combined", ssim_weight=0.0), _trainer(vad, loss="mse")
    la, _ = a.forward_backward(x)
    lb, _ = b.forward_backward(x)
    assert abs(float(la) - float(lb)) < 2e-6 * float(lb), (float(la), float(lb))
    zero_true = R.bn_fed_biases(a.model)
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        if k in zero_true:
            assert float(p.grad.abs().max()) == 0.0 and float(q.grad.abs().max()) == 0.0, k
            continue
        err = float((p.grad - q.grad).abs().max()) / max(float(q.grad.abs().max()), 1e-12)
        assert err < 1e-4, f"{k}: {err:.3e} of the largest entry"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mse_through_the_criterion_entry_is_the_legacy_step(vad, precision):
    """loss_kind 0 of `vad_vid_train_fwd_bwd_l` (what `VideoTrainer(loss="mse")` calls) against `vad_vid_train_fwd_bwd` called
    directly on the same buffers: every output the same bits."""
    l, x = vad.hip.lib(), _clips(vad)
    b, t, _, h, w = x.shape
    tr = _trainer(vad, latent=(32, 64), loss="mse", precision=precision)
    running0 = tr.running.clone()
    loss_new, recon_new = tr.forward_backward(x, recon=True)
    new = (loss_new.clone(), recon_new.clone(), tr.grad.clone(), tr.running.clone())
    tr.running.copy_(running0)
    tr.grad.fill_(NAN)
    nbytes = l.vad_vid_train_workspace_bytes(b, t, h, w, *tr.cfg)
    assert nbytes == l.vad_vid_train_workspace_bytes_l(b, t, h, w, *tr.cfg, 0)
    ws, loss, recon = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), _nan((1,)), _nan(tuple(x.shape))
    vad.hip.check(l.vad_vid_train_fwd_bwd(x.data_ptr(), b, t, h, w, *tr.cfg, tr.flat.data_ptr(), tr.grad.data_ptr(), tr.running.data_ptr(),
                                          ws.data_ptr(), nbytes, vad.hip.precision_mode(tr.precision), loss.data_ptr(), recon.data_ptr(),
                                          vad.hip.current_stream()))
    torch.cuda.synchronize()
    for name, a, c in zip(("loss", "recon", "grads", "running"), new, (loss[0], recon, tr.grad, tr.running)):
        assert torch.equal(a, c), name


def test_criterion_arguments_are_checked(vad):
    m = R.make(vad, 32, 1, 56).cuda()
    with pytest.raises(vad.hip.VadError, match="loss must be one of"):
        vad.VideoTrainer(m, loss="l1")
    x = _clips(vad, b=1, t=2, h=16, w=16)
    for window in (10, 17, 0):
        tr = vad.VideoTrainer(m, loss="ssim", window_size=window)
        tr.grad.fill_(NAN)
        with pytest.raises(vad.hip.VadError, match="window_size"):
            tr.forward_backward(x)
        assert bool(torch.isnan(tr.grad).all())                       # refused before anything ran
    tr = vad.VideoTrainer(m, loss="combined")
    assert (tr.loss, tr.ssim_weight, tr.window_size) == ("combined", 0.5, 11)
    assert vad.VideoTrainer(m).loss == "mse"
    l = vad.hip.lib()
    loss = _nan((1,))
    ws = torch.empty(l.vad_vid_train_workspace_bytes_l(1, 2, 16, 16, *tr.cfg, 2), dtype=torch.uint8, device="cuda")
    rc = l.vad_vid_train_fwd_bwd_l(x.data_ptr(), 1, 2, 16, 16, *tr.cfg, tr.flat.data_ptr(), tr.grad.data_ptr(), tr.running.data_ptr(), ws.data_ptr(),
                                   ws.numel(), 3, 0.5, 11, 0, loss.data_ptr(), None, vad.hip.current_stream())
    assert rc != 0 and b"loss_kind must be 0 (mse), 1 (ssim) or 2 (combined)" in l.vad_last_error()


# ------------------------------------------------------------------------------------------------ 5. loss curve
#: largest relative distance between the fp32 and the float64 CPU trajectory (stock autograd, 4 threads) of the test below, with
#: the test's own weights; measured on the CPU with vid_train_criterion_ref.cpu_trajectory(double=False / True)
CPU_SPREAD = {"ssim": 8.83e-4, "combined": 9.53e-4}
_CPU_CURVES = {}


def _cpu_curve(vad, loss, case, steps, lr):
    if loss not in _CPU_CURVES:
        latent, layers, b, t, hw, wseed = case
        x = torch.from_numpy(vad.synth.clips(wseed + 100, 0, b, t, 3, hw, hw))
        _CPU_CURVES[loss] = R.cpu_trajectory(vad, latent, layers, wseed, x, loss, steps, lr)
    return _CPU_CURVES[loss]


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd", "bf16", "bf16_operands"])
@pytest.mark.parametrize("loss", ["ssim", "combined"])
def test_criterion_loss_curve_follows_cpu_autograd(vad, loss, precision):
    """The gate of test_loss_curve_follows_cpu_autograd_over_many_steps (tests/test_hip_train_step.py) with the SSIM criteria: 25
    Adam steps at lr 1e-3 on one 2x3x32x32 batch, latent 64, two layers, against fp32 CPU autograd of the stock composition
    (CombinedLoss alpha 0.5, window 11).

    Bound, fp32 / split / winograd: the larger of that test's 5e-4 and twice the distance between the fp32 and the float64 CPU
    evaluation of this same trajectory - two correct fp32 evaluations cannot be expected closer to each other than each is to the
    exact one.  Measured on the CPU with these weights (wseed 47): 8.83e-4 for ssim (step 22) and 9.53e-4 for combined (step 12), so
    the bounds are 1.77e-3 and 1.91e-3 (for comparison, the MSE trajectory of these weights: 1.6e-7).  bf16 modes: that test's 2e-2.
    The loss falls: the CPU restatement alone reaches last / first = 0.776 (ssim) and 0.754 (combined) with these weights."""
    case, steps, lr = (64, 2, 2, 3, 32, 47), 25, 1e-3
    latent, layers, b, t, hw, wseed = case
    want = _cpu_curve(vad, loss, case, steps, lr)
    assert want[-1] < 0.8 * want[0], (want[0], want[-1])
    x = torch.from_numpy(vad.synth.clips(wseed + 100, 0, b, t, 3, hw, hw)).cuda()
    tr = vad.VideoTrainer(R.make(vad, latent, layers, wseed).cuda(), lr=lr, weight_decay=WD, precision=precision, loss=loss, ssim_weight=0.5)
    got = [float(tr.step(x)) for _ in range(steps)]
    rel = [abs(a - r) / r for a, r in zip(got, want)]
    bound = 2e-2 if precision.startswith("bf16") else max(5e-4, 2.0 * CPU_SPREAD[loss])
    print(f"[{loss},{precision}] loss curve: max rel deviation {max(rel):.2e} at step {int(np.argmax(rel))} (bound {bound:.2e}); "
          f"{got[0]:.5f} -> {got[-1]:.5f} (cpu {want[-1]:.5f})")
    assert max(rel) < bound, f"loss curves diverge: max rel {max(rel):.2e} at step {int(np.argmax(rel))}: {got[-3:]} vs {want[-3:]}"
    assert got[-1] < 0.8 * got[0], (got[0], got[-1])


# ------------------------------------------------------------------------------------------------ 6. workspace contract
def test_criterion_step_refuses_a_short_workspace_before_any_launch(vad):
    import hip_helpers as H
    l = vad.hip.lib()
    tr = _trainer(vad, latent=(32, 64), loss="combined")
    b, t, h, w = 1, 2, 32, 32
    x = _clips(vad, 4, b, t, h, w)
    size = l.vad_vid_train_workspace_bytes_l(b, t, h, w, *tr.cfg, 2)
    assert size > l.vad_vid_train_workspace_bytes(b, t, h, w, *tr.cfg) > 0
    tr.grad.fill_(NAN)
    loss, recon = _nan((1,)), _nan((b, t, 3, h, w))
    outputs = [tr.grad, tr.running, loss, recon]
    before = [o.clone() for o in outputs]
    arena = H.GuardedArena(size, 0x7F)

    def launch(nbytes):
        return l.vad_vid_train_fwd_bwd_l(x.data_ptr(), b, t, h, w, *tr.cfg, tr.flat.data_ptr(), tr.grad.data_ptr(), tr.running.data_ptr(),
                                         arena.ptr(), nbytes, 2, 0.5, 11, 0, loss.data_ptr(), recon.data_ptr(), vad.hip.current_stream())

    rc = launch(size - 1)
    torch.cuda.synchronize()
    assert rc == -3, f"a workspace of size - 1 bytes returned {rc}: {l.vad_last_error().decode()}"        # VAD_ERR_WS
    for o, keep in zip(outputs, before):
        assert H.same_bits(o, keep), "an output was written by a refused call"
    assert arena.still_poison(), "the workspace was written by a refused call"
    arena.check("refused criterion step")
    assert launch(size) == 0, "the reported size itself is refused"
    arena.check("criterion step")
    assert bool(torch.isfinite(loss).all() and torch.isfinite(tr.grad).all() and torch.isfinite(recon).all())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_criterion_step_ignores_what_the_workspace_held(vad, precision, monkeypatch):
    """Kind 2 at 1x2x32x32 on a workspace of EXACTLY the reported size between two guards, filled with 0x00, 0xFF (NaN in fp32 and
    bf16), 0x7F (3.39e38) and the fp32 quiet NaN: loss, gradients, running statistics and reconstruction are the bits of the plain
    run, with and without a caller's reconstruction buffer, and the guards stay intact."""
    import hip_helpers as H
    l = vad.hip.lib()
    tr = _trainer(vad, latent=(32, 64), loss="combined", precision=precision)
    b, t, h, w = 1, 2, 32, 32
    x = _clips(vad, 4, b, t, h, w)
    running0 = tr.running.clone()

    def call(want_recon):
        tr.running.copy_(running0)
        tr.grad.fill_(NAN)
        loss, recon = tr.forward_backward(x, recon=want_recon)
        torch.cuda.synchronize()
        out = {"loss": loss.clone(), "grads": tr.grad.clone(), "running": tr.running.clone()}
        if want_recon:
            out["recon"] = recon.clone()
        return out

    plain = {flag: call(flag) for flag in (True, False)}
    assert all(bool(torch.isfinite(v).all()) for v in plain[True].values())
    size = l.vad_vid_train_workspace_bytes_l(b, t, h, w, *tr.cfg, 2)
    arena = H.GuardedArena(size, 0x00)

    def ensure(self, nbytes):
        assert nbytes == size
        return arena.body

    monkeypatch.setattr(vad.training._FlatTrainer, "_ensure_ws", ensure)
    for fill in H.POISONS + ("nan",):
        for flag in (True, False):
            if fill == "nan":
                arena.floats().fill_(NAN)
            else:
                arena.poison(fill)
            got = call(flag)
            arena.check(f"criterion step, fill {fill}")
            bad = [k for k in plain[flag] if not H.same_bits(got[k], plain[flag][k])]
            assert not bad, f"{bad} depend on what the workspace held on entry (fill {fill}, recon buffer {flag})"
