"""CPU-only checks of the training-step audit (tests/train_audit_ref.py; the GPU side is tests/test_hip_train_audit.py):

  * the per-launch float64 reference is valid: chained with no rounding it IS the model - loss and every parameter gradient of
    float64 autograd over `VideoAutoencoder` (train mode, MSE) to 1e-10 relative, on the audit's configurations, with the first
    layer's weight gradient in both of its forms;
  * the audit has teeth: a synthetic bf16 workspace trace (the chained reference, rounding where the bf16 mode stores) passes,
    and each seeded defect of the step's address arithmetic is flagged at its launch and nowhere else;
  * the offsets the two debug layout queries report are 64-float aligned, ordered as carved, disjoint and inside the workspace.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import train_audit_ref as R

CONFIGS, IDS, make_case = R.CONFIGS, R.IDS, R.make_case

_CHAINS = {}


def exact_chain(vad, cfg, routed):
    key = (cfg, routed)
    if key not in _CHAINS:
        m, x = make_case(vad, cfg)
        c = R.Cfg(*cfg)
        P, names = R.params_from_model(m)
        mode = R.Mode("exact")
        x64 = x.double().numpy().reshape(c.N, 3, c.H, c.W)
        _CHAINS[key] = (R.chain(R.program(c, mode, P, x64, routed=routed), mode), names, m, x)
    return _CHAINS[key]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_chained_reference_is_float64_autograd(vad, cfg):
    tr, names, m, x = exact_chain(vad, cfg, True)
    m64 = m.double().train()
    loss = nn.MSELoss()(m64(x.double()), x.double())
    loss.backward()
    want = {k: p.grad.detach().numpy() for k, p in m64.named_parameters()}
    assert abs(float(tr["loss"]) - float(loss.detach())) <= 1e-10 * float(loss.detach())
    plain = exact_chain(vad, cfg, False)[0]
    for short, full in names.items():
        g, r = tr["G." + short], want[full]
        assert g.shape == r.shape, short
        scale = np.abs(r).max()
        if short[:3] in ("e_b", "d_b") and short[3].isdigit():       # a bias in front of a batch-statistics BatchNorm: truly zero
            assert not g.any() and scale < 1e-10 * np.abs(want[full.replace("bias", "weight")]).max(), short
            continue
        assert np.abs(g - r).max() <= 1e-10 * scale, f"{short}: {np.abs(g - r).max() / scale:.2e}"
        assert np.abs(plain["G." + short] - r).max() <= 1e-10 * scale, f"{short} (plain first-layer weight gradient)"


# ------------------------------------------------------------------------------------------------ the audit has teeth
TEETH_CFG = CONFIGS[1]          # proj, two layers, B = 2, T = 3, non-square


def _truncate(outs):
    for o in outs:
        if o.kind == "act":
            o.aux = R.trunc_bf16
    return outs


#: name -> (defects for chain(), prefix every flagged launch must carry).  The FIRST flagged launch in program order must be the
#: seeded one.  Two defects are seen by further launches of the same layer, for reasons of the step itself: the dc chain is never
#: stored per step, so the audit carries it in float64 and the steps after a wrong dc disagree with it too; and an h1 store into
#: slab t clobbers what step t-1 stored there and what step t's own convolution read, so the audit can reproduce neither of them
#: from the trace any more (there the seeded launch is flagged, but is not the first).
DEFECTS = {
    "dh2 dropped at t = T-2": ({"lstm_bwd[0,1].gates": {"drop_dh2": True}}, "lstm_bwd[0,"),
    "h of step t written to slab t": ({"lstm_fwd[1,1].state": {"h1_slab": 1}}, "lstm_fwd[1,"),
    "a tensor offset by one channel group": ({"lstm_bwd[1,2].conv_dgrad": {"roll": 4}}, "lstm_bwd[1,2].conv_dgrad"),
    "frame remap left out": ({"enc3.bn_act_pool_fwd": {"remap": False}}, "enc3.bn_act_pool_fwd"),
    "a store truncated, not rounded to nearest even": ({"dec1.bn_act_fwd": _truncate}, "dec1.bn_act_fwd"),
    "the proj output read where hseq is meant": ({"proj.wgrad": {"a_from_pseq": True}}, "proj.wgrad"),
    "a ConvLSTM weight gradient over T-1 steps": ({"lstm_bwd[1].wgrad": {"steps": 2}}, "lstm_bwd[1].wgrad"),
}


@pytest.fixture(scope="module")
def teeth(vad):
    m, x = make_case(vad, TEETH_CFG)
    c = R.Cfg(*TEETH_CFG)
    P, _ = R.params_from_model(m)
    mode = R.Mode("bf16")
    x64 = x.double().numpy().reshape(c.N, 3, c.H, c.W)
    return R.program(c, mode, P, x64), mode


def test_clean_bf16_trace_passes(teeth):
    prog, mode = teeth
    checks = R.audit(prog, R.chain(prog, mode), mode)
    assert R.failing_launches(checks) == [], [ch for ch in checks if not ch.ok]
    assert {name for name, _ in prog} == {ch.launch for ch in checks}          # every launch was reached
    # the synthetic trace is exactly round_bf16(v) wherever the bf16 mode stores: nothing may be off the nearest-even value
    assert max(ch.off_share for ch in checks) == 0.0


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defect_is_flagged_at_its_launch(teeth, defect):
    prog, mode = teeth
    spec, where = DEFECTS[defect]
    assert set(spec) <= {name for name, _ in prog}
    c = R.Cfg(*TEETH_CFG)
    stale = {"cath1_2": np.zeros((c.B, c.h16, c.w16, c.Hd))}          # what the slab nobody wrote still holds
    failing = set(R.failing_launches(R.audit(prog, R.chain(prog, mode, spec, stale), mode)))
    assert failing, f"{defect}: not noticed"
    in_order = [name for name, _ in prog if name in failing]
    seeded, = spec
    assert all(f.startswith(where) for f in failing) and seeded in failing, f"{defect}: flagged {in_order}, seeded at {seeded}"
    if "slab" not in defect:
        assert in_order[0] == seeded, f"{defect}: first flagged {in_order[0]}, seeded at {seeded}"


def test_number_format_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0078125, 0.0, 1e-20, 257.0, 258.0])
    want = torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).double().numpy()      # torch rounds to nearest even too
    assert np.array_equal(R.round_bf16(v), want)
    assert np.array_equal(R.spacing_bf16([1.0, 1.99, 2.0, 0.75]), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8])
    assert np.array_equal(R.trunc_bf16([1.0078124, -1.0078124]), [1.0, -1.0])


# ------------------------------------------------------------------------------------------------ layout arithmetic
@pytest.mark.parametrize("loss_kind", [0, 2])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_debug_layouts_are_aligned_ordered_disjoint_and_inside(vad, cfg, loss_kind):
    lib = vad.hip.lib()
    c = R.Cfg(*cfg)
    lay, total = R.workspace_layout(lib, c, loss_kind)
    nbytes = lib.vad_vid_train_workspace_bytes_l(c.B, c.T, c.H, c.W, c.L, c.Hd, c.NL, loss_kind)
    assert nbytes == 4 * total > 0
    live = {k: v for k, v in lay.items() if v[1] > 0}
    assert ("pseq" in live) == c.proj and ("recon" in live) == ("drecon" in live) == (loss_kind != 0)
    for k, (off, sz) in lay.items():
        assert (off == 0) == (k not in live), f"{k}: an absent buffer reports offset 0, a live one never"
    spans = sorted((off, off + sz, k) for k, (off, sz) in live.items())
    for off, end, k in spans:
        assert off % 64 == 0 and end <= total, (k, off, end, total)
    for (o0, e0, k0), (o1, e1, k1) in zip(spans, spans[1:]):
        assert e0 <= o1, f"{k0} [{o0}, {e0}) overlaps {k1} [{o1}, {e1})"
    # the carve order of csrc/train_step.hip: per encoder stage, per ConvLSTM layer, the dc buffers, hseq / pseq, per decoder
    # stage, dpre, the gradient scratch g0, g2, g1, the k sums and - behind everything else - the criterion's buffers
    order = [k for _, _, k in spans]
    want = []
    for k in range(4):
        want += [f"y{k}"] + ([f"a{k}"] if k < 3 else []) + [f"st_e{k}"]
    for l in range(c.NL):
        want += [f"cat{l}", f"z{l}", f"c{l}", f"dcat{l}", f"dzl{l}"]
    want += [f"dc{l}" for l in range(c.NL)] + ["hseq"] + (["pseq"] if c.proj else [])
    for j in range(3):
        want += [f"u{j}", f"r{j}", f"st_d{j}"]
    want += ["dpre", "g0", "g2", "g1", "ksums"] + (["recon", "drecon"] if loss_kind else [])
    assert order == want
