"""Per-frame SSIM / combined scores and SSIM maps in one scoring pass: vad_ssim_score (csrc/ssim.hip), `losses.ssim_per_frame`,
`score_criteria` of both models and `scoring.validate`.

Bounds, and where they come from:
* 2e-6 on a per-frame value computed from the golden's own inputs: what test_ssim_combined_losses_match_reference_golden holds
  the same arithmetic to (the reference's fp32 per-frame values sit within 7e-7 of float64);
* 1e-5 (relative, the project's score gate SCORE_RTOL) through a model: a 1e-6 change of the reconstruction moves a per-frame
  SSIM by <= 6e-8;
* 1e-5 on a per-frame value against the float64 composition at ragged sizes;
* the per-pixel map has NO constant bound: E[x^2] - mu^2 cancels in fp32 over the C2 = 9e-4 floor, so the kernel's distance
  from float64 is held to 4 x the distance of the reference's own fp32 composition on the same inputs + 2e-6 (4: the separable
  fmaf order against conv2d's 2-D window).
The 2e-6 gate needs inputs on which the reference's own fp32 value is that good: it is (<= 9e-7 from float64) on every golden,
the low-contrast one included (0.8 + 0.01 * noise frames against a model's reconstruction).  On a pair where BOTH sides are such
frames the reference itself is 5e-6 (window 11) to 1e-5 (window 15) from float64; that pair is built in the map test, whose
bound scales with exactly this error.  Everything else is bit identity."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_synthetic, max_abs, rel_err
from ssim_score_ref import ssim_frames

REPO = Path(__file__).resolve().parent.parent
GOLD = "ssim_score/"
NEW_SYMBOLS = ["vad_ssim_score_workspace_floats", "vad_ssim_score"]
ERR_ARG = -1
SCORE_RTOL = 1e-5         # the project's score gate (tests/test_hip_models.py SCORE_RTOL)
KERNEL_ATOL = 2e-6
GEOM_ATOL = 1e-5
NAN = float("nan")


# ------------------------------------------------------------------------------ CPU
def test_every_ssim_score_fixture_has_a_generator():
    """tests/golden/ssim_score/*.npz are captured from the reference by make_golden_ssim_score.py: every committed fixture is
    one that script regenerates, and vice versa."""
    import ast
    here = REPO / "tests" / "golden" / "ssim_score"
    names = set()
    for node in ast.walk(ast.parse((here / "make_golden_ssim_score.py").read_text())):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "FIXTURES" for t in node.targets):
            names = {k.value for k in node.value.keys}
    assert names and names == {p.name for p in here.glob("*.npz")}


def test_signatures_bind_both_symbols(vad):
    header = (REPO / "include" / "vad_hip.h").read_text()
    lib = vad.hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/vad_hip.h"
        assert name in vad.hip.SIGNATURES and hasattr(lib, name)
    assert lib.vad_abi_version() == 3


def test_workspace_query_without_gpu(vad):
    q = vad.hip.lib().vad_ssim_score_workspace_floats
    assert q(5, 48, 80) == 5 * 2 * 3 and q(1, 7, 5) == 1 and q(2, 33, 64) == 2 * 2 * 2
    for shape in [(0, 32, 32), (-1, 32, 32), (1, 0, 32), (1, 32, 0), (1, -4, 32), (1, 32, -4)]:
        assert q(*shape) == 0
    assert q(1 << 31, 32, 32) == 0                         # the launch grid would not fit
    assert q((1 << 31) - 1, 32, 32) == (1 << 31) - 1
    assert q(1 << 40, 1 << 20, 1 << 20) == 0 and q(1 << 62, 64, 64) == 0 and q((1 << 63) - 1, 33, 33) == 0      # no wrapped product
    assert q((1 << 29) - 1, 64, 64) == 4 * ((1 << 29) - 1) and q(1 << 29, 64, 64) == 0                           # the launch's own limit


def test_refusals_without_gpu(vad):
    """Every argument error of vad_ssim_score is reported before anything is launched: on a machine without a GPU, with
    pointers that are never dereferenced."""
    lib = vad.hip.lib()
    buf = (C.c_float * 4)()
    p = C.addressof(buf)

    def call(recon=p, x=p, fmt=0, frames=1, c=3, h=32, w=32, window=11, mse=None, ws=p, ssim=p, comb=None, smap=None):
        rc = lib.vad_ssim_score(recon, x, fmt, frames, c, h, w, window, 0.5, mse, ws, ssim, comb, smap, None)
        return rc, lib.vad_last_error().decode()

    for kw in (dict(recon=None), dict(x=None), dict(ws=None), dict(ssim=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "null pointer" in msg, (kw, msg)
    rc, msg = call(comb=p)
    assert rc == ERR_ARG and "mse_in" in msg
    for c in (1, 4):
        rc, msg = call(fmt=vad.hip.X_U8_NHWC, c=c)
        assert rc == ERR_ARG and "uint8" in msg and f"c={c}" in msg
    rc, msg = call(fmt=7)
    assert rc == ERR_ARG and "x_format" in msg
    for window in (0, 2, 10, 17, -3):
        rc, msg = call(window=window)
        assert rc == ERR_ARG and "window_size" in msg, window
    for kw in (dict(frames=0), dict(c=0), dict(h=0), dict(w=-1)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "shape" in msg, kw
    rc, msg = call(frames=1 << 31)
    assert rc == ERR_ARG and "grid too large" in msg
    rc, msg = call(frames=1 << 40, h=1 << 20, w=1 << 20)
    assert rc == ERR_ARG and "grid too large" in msg
    rc, msg = call(frames=1 << 29, h=64, w=64)                 # exactly where the size query starts to answer 0
    assert rc == ERR_ARG and "grid too large" in msg


def test_python_refusals_without_gpu(vad):
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(vad.hip.VadError, match="GPU"):
        vad.losses.ssim_per_frame(x, x)
    with pytest.raises(vad.hip.VadError, match="GPU"):
        vad.losses.ssim_per_frame(x, x.numpy())
    with pytest.raises(vad.hip.VadError, match="criterion"):
        vad.scoring.validate(vad.ConvAutoencoder(latent_dim=32), [], "cpu", criterion="l1")
    for m in (vad.ConvAutoencoder(latent_dim=32), vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32)):
        with pytest.raises(vad.hip.VadError, match="inference entry point"):
            m.train().score_criteria(x)


def test_float64_composition_matches_reference_goldens(golden):
    """The yardstick of the geometry and map tests against the reference's own per-sample values."""
    for name in ("img_c3_48x80.npz", "img_c1_32.npz", "img_c5_16.npz", "img_lowcontrast_32x48.npz"):
        g = golden(GOLD + name)
        for win in g["windows"]:
            ssim, _ = ssim_frames(g["recon"], g["x"], int(win))
            assert max_abs(ssim.numpy(), g[f"ssim_w{win}"]) < KERNEL_ATOL, (name, win)


# ------------------------------------------------------------------------------ GPU plumbing
gpu = pytest.mark.gpu


def _kernel(vad, recon, x, window, alpha=0.5, mse=None, want_map=True, ws=None):
    """vad_ssim_score through the C ABI on device tensors; outputs NaN-prefilled -> dict of device tensors."""
    import hip_helpers as H
    l = vad.hip.lib()
    n, c, h, w = recon.shape
    u8 = x.dtype == torch.uint8
    nws = l.vad_ssim_score_workspace_floats(n, h, w)
    assert nws == n * ((h + 31) // 32) * ((w + 31) // 32)
    if ws is None:
        ws = torch.empty(nws, device="cuda")
    out = {"ssim": torch.full((n,), NAN, device="cuda")}
    if mse is not None:
        out["combined"] = torch.full((n,), NAN, device="cuda")
    if want_map:
        out["ssim_map"] = torch.full((n, 1, h, w), NAN, device="cuda")
    vad.hip.check(l.vad_ssim_score(recon.data_ptr(), x.data_ptr(), vad.hip.X_U8_NHWC if u8 else vad.hip.X_F32_NCHW, n, c, h, w, window,
                                   alpha, vad.hip.ptr(mse), ws.data_ptr(), out["ssim"].data_ptr(), vad.hip.ptr(out.get("combined")),
                                   vad.hip.ptr(out.get("ssim_map")), H.stream()), "vad_ssim_score")
    torch.cuda.synchronize()
    return out


def _pair(seed, n, c, h, w):
    """A prediction that resembles its target (SSIM well inside (0, 1)), both in [-1, 1]."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (n, c, h, w)).astype(np.float32)
    p = (0.75 * t + 0.25 * rng.uniform(-1, 1, (n, c, h, w))).astype(np.float32)
    return p, t


# ------------------------------------------------------------------------------ 1. kernel alone
@gpu
@pytest.mark.parametrize("name", ["img_c3_48x80.npz", "img_c1_32.npz", "img_c5_16.npz", "img_lowcontrast_32x48.npz"])
def test_kernel_on_golden_inputs(vad, golden, name):
    import hip_helpers as H
    g = golden(GOLD + name)
    recon, x, mse = H.dev(g["recon"]), H.dev(g["x"]), H.dev(g["mse"])
    for win in g["windows"]:
        out = _kernel(vad, recon, x, int(win), float(g["alpha"]), mse)
        d_ssim, d_comb = max_abs(out["ssim"].cpu().numpy(), g[f"ssim_w{win}"]), max_abs(out["combined"].cpu().numpy(), g[f"combined_w{win}"])
        print(f"{name} window {win}: ssim {d_ssim:.2e} combined {d_comb:.2e}")
        assert d_ssim < KERNEL_ATOL and d_comb < KERNEL_ATOL


# ------------------------------------------------------------------------------ 2. through the models
def _img_model(vad, g):
    m = vad.ConvAutoencoder(in_channels=int(g["in_channels"]), latent_dim=int(g["latent_dim"]))
    load_synthetic(vad, m, int(g["wseed"]))
    return m.cuda().eval()


@gpu
@pytest.mark.parametrize("name", ["img_c3_48x80.npz", "img_c1_32.npz", "img_c5_16.npz", "img_lowcontrast_32x48.npz"])
def test_image_score_criteria_matches_reference(vad, golden, name):
    g = golden(GOLD + name)
    m = _img_model(vad, g)
    x = torch.from_numpy(g["x"]).cuda()
    n0, s0 = vad.hip.calls["img_score"], vad.hip.calls.get("ssim_score", 0)
    with torch.no_grad():
        for win in g["windows"]:
            out = m.score_criteria(x, window_size=int(win), alpha=float(g["alpha"]), ssim_map=True, errmap=True, recon=True)
            assert rel_err(out["mse"].cpu().numpy(), g["mse"]) < SCORE_RTOL
            assert rel_err(out["ssim"].cpu().numpy(), g[f"ssim_w{win}"]) < SCORE_RTOL
            assert rel_err(out["combined"].cpu().numpy(), g[f"combined_w{win}"]) < SCORE_RTOL
            assert out["ssim_map"].shape == (len(x), 1) + x.shape[2:] and out["recon"].shape == x.shape
            assert max_abs(out["ssim_map"].mean(dim=(1, 2, 3)).cpu().numpy(), out["ssim"].cpu().numpy()) < KERNEL_ATOL
        assert vad.hip.calls["img_score"] == n0 + len(g["windows"]) and vad.hip.calls["ssim_score"] == s0 + len(g["windows"])
        assert torch.equal(out["mse"], m.get_reconstruction_error(x))
        assert torch.equal(out["errmap"], m.get_reconstruction_error(x, per_pixel=True))
        assert torch.equal(out["recon"], m(x))
        assert sorted(m.score_criteria(x)) == ["combined", "mse", "ssim"]


@gpu
def test_image_score_criteria_uint8_is_its_normalised_copy(vad, golden):
    g = golden(GOLD + "img_c3_48x80.npz")
    m = _img_model(vad, g)
    u8 = torch.from_numpy(np.ascontiguousarray(vad.synth.frames_u8(17, 0, 3, 3, 48, 80).transpose(0, 2, 3, 1))).cuda()
    xf = torch.from_numpy(vad.synth.frames(17, 0, 3, 3, 48, 80)).cuda()
    with torch.no_grad():
        a, b = m.score_criteria(u8, ssim_map=True), m.score_criteria(xf, ssim_map=True)
    for k in ("mse", "ssim", "combined", "ssim_map"):
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
def test_video_score_criteria(vad, golden, precision):
    g = golden(GOLD + "vid_l32_32.npz")
    b, t, hw = int(g["b"]), int(g["t"]), int(g["hw"])
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=int(g["latent_dim"]), lstm_hidden_dim=int(g["hid"]), lstm_num_layers=int(g["layers"]))
    load_synthetic(vad, m, int(g["wseed"]))
    m = m.cuda().eval()
    m.precision = precision
    x = torch.from_numpy(vad.synth.clips(int(g["xseed"]), 0, b, t, 3, hw, hw)).cuda()
    with torch.no_grad():
        out = m.score_criteria(x, window_size=int(g["window"]), alpha=float(g["alpha"]), ssim_map=True)
        assert torch.equal(out["seq_mse"], m.get_reconstruction_error(x))
        assert torch.equal(out["mse"], m.get_reconstruction_error(x, per_frame=True))
    assert out["ssim_map"].shape == (b, t, 1, hw, hw)
    for k in ("mse", "ssim", "combined"):
        assert out[k].shape == (b, t) and out["seq_" + k].shape == (b,)
    for k in ("ssim", "combined"):
        assert torch.equal(out["seq_" + k], out[k].mean(dim=1))
    # the SSIM kernel is fp32 in every mode: it is the per-frame criterion of that mode's own reconstruction
    with torch.no_grad():
        recon = m(x)
    own = vad.losses.ssim_per_frame(recon.reshape(b * t, 3, hw, hw), x.reshape(b * t, 3, hw, hw), int(g["window"]), float(g["alpha"]),
                                    mse=out["mse"].reshape(-1), ssim_map=True)
    for k in ("ssim", "combined", "ssim_map"):
        assert torch.equal(own[k].reshape(out[k].shape), out[k]), k
    if precision == "fp32":                      # (the other modes are other arithmetic in the forward, gated by their own tests)
        for k in ("mse", "ssim", "combined", "seq_mse", "seq_ssim", "seq_combined"):
            assert rel_err(out[k].cpu().numpy(), g[k]) < SCORE_RTOL, k


@gpu
def test_video_score_criteria_uint8_is_its_normalised_copy(vad, golden):
    g = golden(GOLD + "vid_l32_32.npz")
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=int(g["latent_dim"]), lstm_hidden_dim=int(g["hid"]), lstm_num_layers=int(g["layers"]))
    load_synthetic(vad, m, int(g["wseed"]))
    m = m.cuda().eval()
    u8 = vad.synth.frames_u8(19, 0, 6, 3, 32, 48)                               # 2 clips x 3 frames, 32 x 48: two tiles per frame
    xu = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1)).reshape(2, 3, 32, 48, 3)).cuda()
    xf = torch.from_numpy(vad.synth.u8_to_unit(u8).reshape(2, 3, 3, 32, 48)).cuda()
    with torch.no_grad():
        a, b = m.score_criteria(xu, ssim_map=True), m.score_criteria(xf, ssim_map=True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["ssim_map"].shape == (2, 3, 1, 32, 48)


def _loader(vad, g, key):
    labels, s, batches = g["labels"], 0, []
    for k in g["batches"]:
        k = int(k)
        if key == "image":
            x = vad.synth.frames(int(g["xseed"]), s, k, 3, int(g["hw"]), int(g["hw"]))
        else:
            x = vad.synth.clips(int(g["xseed"]), s, k, int(g["t"]), 3, int(g["hw"]), int(g["hw"]))
        batches.append({key: torch.from_numpy(x), "label": torch.from_numpy(labels[s:s + k])})
        s += k
    return batches


@gpu
@pytest.mark.parametrize("kind", ["img", "vid"])
def test_validate_matches_reference_loop(vad, golden, kind):
    g = golden(GOLD + f"validate_{kind}.npz")
    if kind == "img":
        m = vad.ConvAutoencoder(latent_dim=int(g["latent_dim"]))
    else:
        m = vad.VideoAutoencoder(latent_dim=int(g["latent_dim"]), lstm_hidden_dim=int(g["hid"]), lstm_num_layers=int(g["layers"]))
    load_synthetic(vad, m, int(g["wseed"]))
    m = m.cuda()
    loader = _loader(vad, g, "image" if kind == "img" else "frames")
    for crit in ("mse", "ssim", "combined"):
        n0 = vad.hip.calls["img_score" if kind == "img" else "vid_score"]
        got = vad.scoring.validate(m, loader, "cuda", criterion=crit)
        assert vad.hip.calls["img_score" if kind == "img" else "vid_score"] == n0 + len(loader)      # one forward per batch
        assert len(got) == 3 and rel_err(np.array(got, dtype=np.float64), g[crit]) < SCORE_RTOL, (crit, got, g[crit])


# ------------------------------------------------------------------------------ 3. exactness
@gpu
def test_frame_value_does_not_depend_on_the_batch(vad, golden):
    import hip_helpers as H
    g = golden(GOLD + "img_c3_48x80.npz")
    recon, x, mse = H.dev(g["recon"]), H.dev(g["x"]), H.dev(g["mse"])
    whole = _kernel(vad, recon, x, 11, 0.3, mse)
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    mixed = _kernel(vad, recon[perm].contiguous(), x[perm].contiguous(), 11, 0.3, mse[perm].contiguous())
    for k in whole:
        assert torch.equal(mixed[k], whole[k][perm]), k
    for i in range(5):
        alone = _kernel(vad, recon[i:i + 1].contiguous(), x[i:i + 1].contiguous(), 11, 0.3, mse[i:i + 1].contiguous())
        for k in whole:
            assert torch.equal(alone[k], whole[k][i:i + 1]), (k, i)
    # without a map / without the combination the other outputs are the same bits
    assert torch.equal(_kernel(vad, recon, x, 11, 0.3, None, want_map=False)["ssim"], whole["ssim"])


@gpu
@pytest.mark.parametrize("window", [3, 11])
def test_uint8_input_is_its_normalised_copy(vad, window):
    import hip_helpers as H
    u8 = vad.synth.frames_u8(23, 0, 3, 3, 37, 53)
    xf = H.dev(vad.synth.u8_to_unit(u8))
    xu = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).cuda()
    recon = H.dev(_pair(5, 3, 3, 37, 53)[0])
    mse = ((recon - xf) ** 2).mean(dim=(1, 2, 3))
    a, b = _kernel(vad, recon, xu, window, 0.5, mse), _kernel(vad, recon, xf, window, 0.5, mse)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    out = vad.losses.ssim_per_frame(recon, xu, window, 0.5, mse=mse, ssim_map=True)
    for k in a:
        assert torch.equal(out[k], a[k]), k


@gpu
def test_consistency_with_the_batch_criterion(vad, golden):
    import hip_helpers as H
    g = golden(GOLD + "img_c3_48x80.npz")
    recon, x, mse = H.dev(g["recon"]), H.dev(g["x"]), H.dev(g["mse"])
    n0 = vad.hip.calls.get("ssim_score", 0)
    out = vad.losses.ssim_per_frame(recon, x, 11, 0.3, mse=mse, ssim_map=True)
    assert vad.hip.calls["ssim_score"] == n0 + 1
    assert max_abs(out["ssim_map"].mean(dim=(1, 2, 3)).cpu().numpy(), out["ssim"].cpu().numpy()) < KERNEL_ATOL
    batch = float(vad.SSIMLoss(window_size=11)(recon, x))           # vad_ssim_mse over the whole batch
    assert abs(float(out["ssim"].mean()) - batch) < KERNEL_ATOL
    assert torch.allclose(out["combined"], (1 - 0.3) * mse + 0.3 * out["ssim"], rtol=1e-6)
    assert sorted(vad.losses.ssim_per_frame(recon, x)) == ["ssim"]


# ------------------------------------------------------------------------------ 4. ragged geometry
SIZES = [(7, 5), (33, 64), (37, 53), (32, 32)]      # 32 x 32 tiles: cut by the edge on one or both axes, and exact


@gpu
@pytest.mark.parametrize("window", [1, 3, 11, 15])
@pytest.mark.parametrize("size", SIZES)
def test_ragged_geometry_against_float64(vad, size, window):
    import hip_helpers as H
    h, w = size
    for c in (1, 3, 5):
        p, t = _pair(1000 * h + 10 * window + c, 2, c, h, w)
        want, want_map = ssim_frames(p, t, window)
        out = _kernel(vad, H.dev(p), H.dev(t), window)
        d = max_abs(out["ssim"].cpu().numpy(), want.numpy())
        assert d < GEOM_ATOL, (size, window, c, d)
        ref_dev = max_abs(ssim_frames(p, t, window, torch.float32)[1].numpy(), want_map.numpy())
        assert max_abs(out["ssim_map"].cpu().numpy(), want_map.numpy()) <= 4 * ref_dev + 2e-6       # (the rule of test 5)


# ------------------------------------------------------------------------------ 5. per-pixel map
def _map_inputs(golden, kind):
    if kind == "uniform":
        g = golden(GOLD + "img_c3_48x80.npz")
        return g["recon"], g["x"]
    if kind == "lowcontrast":                         # the model's reconstruction of 0.8 + 0.01 * noise frames
        g = golden(GOLD + "img_lowcontrast_32x48.npz")
        return g["recon"], g["x"]
    if kind == "lowcontrast_pair":                    # BOTH sides 0.8 + 0.01 * noise: every variance term cancels over the C2 floor
        rng = np.random.default_rng(311)
        return tuple((0.8 + 0.01 * rng.standard_normal((3, 3, 32, 48))).astype(np.float32) for _ in range(2))
    if kind == "smooth":
        yy, xx = np.meshgrid(np.linspace(-1, 1, 37), np.linspace(-1, 1, 53), indexing="ij")
        t = np.stack([np.sin(2 * yy + ch) * np.cos(3 * xx - ch) for ch in range(3)])[None].astype(np.float32)
        return (0.9 * t + 0.05).astype(np.float32), t
    p = np.full((2, 3, 33, 40), 0.7, np.float32)        # constant frames: zero variance, pure cancellation over C2
    return p, np.full_like(p, 0.65)


@gpu
@pytest.mark.parametrize("window", [3, 11, 15])
@pytest.mark.parametrize("kind", ["uniform", "lowcontrast", "lowcontrast_pair", "smooth", "constant"])
def test_map_deviation_is_bounded_by_the_conditioning(vad, golden, kind, window):
    import hip_helpers as H
    p, t = _map_inputs(golden, kind)
    _, m64 = ssim_frames(p, t, window, torch.float64)
    _, m32 = ssim_frames(p, t, window, torch.float32)
    got = _kernel(vad, H.dev(p), H.dev(t), window)["ssim_map"].cpu().numpy()
    ref_dev, dev = max_abs(m32.numpy(), m64.numpy()), max_abs(got, m64.numpy())
    print(f"map {kind} window {window}: fp32 composition {ref_dev:.3e}, kernel {dev:.3e}, ratio {dev / max(ref_dev, 1e-30):.2f}")
    assert dev <= 4 * ref_dev + 2e-6


# ------------------------------------------------------------------------------ 6. workspace contract
@gpu
@pytest.mark.parametrize("size", SIZES)
def test_workspace_contract(vad, size):
    import hip_helpers as H
    h, w = size
    p, t = _pair(7 * h + w, 3, 3, h, w)
    recon, x = H.dev(p), H.dev(t)
    mse = ((recon - x) ** 2).mean(dim=(1, 2, 3))
    nws = vad.hip.lib().vad_ssim_score_workspace_floats(3, h, w)
    plain = _kernel(vad, recon, x, 11, 0.5, mse)
    assert all(bool(torch.isfinite(v).all()) for v in plain.values())
    for fill in H.POISONS:
        pool = H.ArenaPool(fill)
        got = _kernel(vad, recon, x, 11, 0.5, mse, ws=pool.new(4 * nws, "vad_ssim_score workspace").floats())
        pool.check()
        bad = [k for k in plain if not H.same_bits(got[k], plain[k])]
        assert not bad, f"{h}x{w}: {bad} depend on the workspace (fill 0x{fill:02X})"
