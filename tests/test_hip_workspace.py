"""The workspace contract of include/vad_hip.h: a caller-supplied workspace is device scratch - its contents on entry are
irrelevant, and no byte outside [ws, ws + size) is read or written.

Every case runs one entry point four times: once through the ordinary Python path (a `torch.empty` workspace, as every other
test and the product use), and three times on a `hip_helpers.GuardedArena` whose body is EXACTLY the number of bytes the
library's size function reports, between two 1 MiB guards, filled with 0x00 (zero: hides "assumed cleared"), 0xFF (NaN in fp32
and bf16) and 0x7F (3.39e38: a stale NaN can be swallowed by max / ReLU / max-pool, a huge finite value cannot).  Every output
must be the SAME BITS in all four runs and both guards must be untouched.  There is no tolerance anywhere in this file: the
accuracy tests of the other files then hold for any workspace contents.

The models' and trainers' only allocation points (`_HipScorer.workspace`, `_FlatTrainer._ensure_ws`) are monkeypatched per test
to hand out arena bodies; criteria, resize and the refusals go through the C ABI directly.  Shapes are the smallest at which
the carving of a workspace can still disagree with its size function."""
import hashlib
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_synthetic

pytestmark = pytest.mark.gpu

NAN = float("nan")
ERR_WS = -3


# ------------------------------------------------------------------------------ plumbing
def _inject(vad, mp, pool):
    """Route the two allocation points of the model / trainer classes to `pool` (one arena per distinct size)."""
    mp.setattr(vad.autoencoder._HipScorer, "workspace", lambda self, nbytes, device: pool.shared(nbytes))
    mp.setattr(vad.training._FlatTrainer, "_ensure_ws", lambda self, nbytes: pool.shared(nbytes))


def _flat(out, prefix=""):
    """Every tensor of a nested result (dict / list / tuple / VideoState) under a readable name."""
    if out is None:
        return {}
    if isinstance(out, torch.Tensor):
        return {prefix or "out": out}
    if hasattr(out, "blob"):
        return {prefix + ".state": out.blob}
    items = out.items() if isinstance(out, dict) else enumerate(out)
    res = {}
    for k, v in items:
        res.update(_flat(v, f"{prefix}.{k}" if prefix else str(k)))
    return res


def _finite(name, t, label):
    if t.is_floating_point():
        assert bool(torch.isfinite(t).all()), f"{label}: {name} of the plain run is not finite"


def _same_as_recorded(label, plain):
    """Scoring has no atomics: every output of a scoring case is the bits an MI355X gave before the workspaces were laid out by
    one carve each (tests/golden/scoring_digests.json names the commit)."""
    want = json.loads((GOLDEN / "scoring_digests.json").read_text())["sha256"]
    got = {k: hashlib.sha256(v.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for k, v in plain.items()}
    assert got == want[label], f"{label}: {[k for k in got if got[k] != want[label].get(k)]} are not the recorded bits"


def _contract(vad, call, label, plain=None, recorded=True):
    """`call()` -> nested tensors.  Plain run, then the three fills on guarded arenas: same bits, clean guards.  The plain run of
    a scoring case (`plain` not given) is also compared with its recorded digests."""
    import hip_helpers as H
    if plain is None:
        with torch.no_grad():
            plain = {k: v.clone() for k, v in _flat(call()).items()}
        if recorded:
            _same_as_recorded(label, plain)
    torch.cuda.synchronize()
    assert plain, label
    for k, v in plain.items():
        _finite(k, v, label)
    pool = H.ArenaPool()
    with pytest.MonkeyPatch.context() as mp:
        _inject(vad, mp, pool)
        for fill in H.POISONS:
            pool.poison(fill)
            with torch.no_grad():
                got = _flat(call())
            pool.check()
            assert pool.by_size, f"{label}: the call asked for no workspace"
            assert sorted(got) == sorted(plain), label
            bad = [k for k in plain if not H.same_bits(got[k], plain[k])]
            assert not bad, f"{label}: {bad} depend on what the workspace held on entry (fill 0x{fill:02X})"
    return pool


_MODELS = {}


def _img_model(vad, cin, latent, precision, chunk):
    key = ("img", cin, latent)
    if key not in _MODELS:
        m = vad.ConvAutoencoder(in_channels=cin, latent_dim=latent)
        load_synthetic(vad, m, 40 + cin + latent)
        _MODELS[key] = m.cuda().eval()
    m = _MODELS[key]
    m.precision, m.chunk = precision, chunk
    return m


def _vid_model(vad, cin, latent, hid, layers, precision, chunk):
    key = ("vid", cin, latent, hid, layers)
    if key not in _MODELS:
        m = vad.VideoAutoencoder(in_channels=cin, latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=layers)
        load_synthetic(vad, m, 70 + cin + latent + hid + layers)
        _MODELS[key] = m.cuda().eval()
    m = _MODELS[key]
    m.precision, m.chunk, m.window_chunk = precision, chunk, chunk
    return m


def _to_u8(x):
    """[-1, 1] float NCHW / NTCHW numpy -> uint8 channel-last device tensor."""
    u8 = np.clip(np.round((x * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(u8, -3, -1))).cuda()


# ------------------------------------------------------------------------------ image scoring
def _img_call(m, x, what):
    if what == "scores":
        return lambda: {"scores": m.get_reconstruction_error(x)}
    if what == "latent":                       # the decoder is skipped
        return lambda: {"latent": m.get_latent(x)}
    return lambda: m._run_hip(x, scores=True, errmap=True, recon=True, latent=True)


SIZES = [(16, 16), (16, 48), (32, 16)]          # one latent pixel; a row of three; a column of two
PRECS = ["fp32", "split", "winograd"]           # (winograd: enc1.0 unfused, a full H x W x 32 map)
IMG_CASES = []
for i, (h, w) in enumerate(SIZES):
    for j, prec in enumerate(PRECS):
        IMG_CASES.append((3, (32, 100)[(i + j) % 2], h, w, 5, 2, prec, "all", False))         # b = 5, chunk = 2: a ragged last group
for j, prec in enumerate(PRECS):
    IMG_CASES.append((3, (100, 32)[j % 2], 16, 16, 5, 2, prec, "all", False))                 # (the other width at one latent pixel)
    IMG_CASES.append((1, 32, 16, 48, 5, 2, prec, "all", False))                               # zero-widened to 3 planes
    IMG_CASES.append((5, 32, 16, 48, 5, 2, prec, "all", False))                               # wide_io: padded planes, own partial count
    IMG_CASES.append((3, 100, 32, 16, 3, 8, prec, "all", False))                              # chunk >= b
IMG_CASES += [(3, 32, 16, 48, 5, 2, "fp32", "scores", False), (3, 100, 32, 16, 5, 2, "winograd", "scores", False),
              (3, 100, 16, 48, 5, 2, "fp32", "latent", False), (3, 32, 32, 16, 5, 2, "winograd", "latent", False),
              (5, 100, 32, 16, 5, 2, "fp32", "scores", False), (5, 32, 16, 16, 3, 8, "split", "latent", False),
              (3, 32, 16, 48, 5, 2, "fp32", "all", True), (3, 100, 32, 16, 5, 2, "split", "all", True),
              (3, 32, 16, 16, 3, 8, "winograd", "scores", True)]


@pytest.mark.parametrize("cin,latent,h,w,b,chunk,precision,what,u8", IMG_CASES)
def test_image_scoring_workspace(vad, cin, latent, h, w, b, chunk, precision, what, u8):
    m = _img_model(vad, cin, latent, precision, chunk)
    x = vad.synth.frames(900 + h + w, 0, b, cin, h, w)
    x = _to_u8(x) if u8 else torch.from_numpy(x).cuda()
    _contract(vad, _img_call(m, x, what), f"image cin {cin} latent {latent} {h}x{w} b {b} chunk {chunk} {precision} {what} u8 {u8}")


@pytest.mark.parametrize("tail_group", [0, 1])
def test_image_scoring_workspace_unfused_tail(vad, tail_group):
    """The two-launch tail (vad_debug_set_dec4_fused(0)) and its per-frame sub-groups index the partial sums differently."""
    l = vad.hip.lib()
    m = _img_model(vad, 3, 32, "fp32", 2)
    x = torch.from_numpy(vad.synth.frames(77, 0, 5, 3, 16, 48)).cuda()
    try:
        l.vad_debug_set_dec4_fused(0)
        l.vad_debug_set_tail_group(tail_group)
        _contract(vad, _img_call(m, x, "all"), f"image, unfused tail, tail group {tail_group}")
    finally:
        l.vad_debug_set_dec4_fused(1)
        l.vad_debug_set_tail_group(0)


def test_image_scoring_workspace_wide_latent(vad):
    """latent_dim just above 2048 at 16 x 16: the enc4.0 output (2 x 2 x 2080) is larger than the H x W x 32 maps, the only way to
    the `e4 > m` branch of the activation size."""
    torch.manual_seed(7)
    m = vad.ConvAutoencoder(latent_dim=2049).cuda().eval()          # (as initialised: a synthetic state of 38 M values takes seconds)
    m.chunk = 2
    x = torch.from_numpy(vad.synth.frames(78, 0, 3, 3, 16, 16)).cuda()
    _contract(vad, _img_call(m, x, "all"), "image latent 2049 16x16", recorded=False)       # (weights as torch initialises them)


# ------------------------------------------------------------------------------ video scoring
VSIZES = [(16, 16), (16, 32), (48, 32)]
VCFG = [(32, 32), (32, 64), (100, 100), (64, 128)]       # (latent, hid): hid != latent has `proj`; 100 pads to 128
VID_CASES = []      # (cin, latent, hid, layers, h, w, b, t, chunk, precision, u8); b = 3, chunk = 2: ragged, below the threshold
k = 0
for latent, hid in VCFG:
    for layers in (1, 2, 3):
        h, w = VSIZES[k % 3]
        t = (1, 3)[(k // 3 + k) % 2]
        VID_CASES.append((3, latent, hid, layers, h, w, 3, t, 2, "fp32", False))
        if layers > 1:                           # (one z buffer per layer; a one-layer case follows below)
            h, w = VSIZES[(k + 1) % 3]
            VID_CASES.append((3, latent, hid, layers, h, w, 3, 4 - t, 2, "winograd", False))
        if hid == latent:
            h, w = VSIZES[(k + 2) % 3]
            VID_CASES.append((3, latent, hid, layers, h, w, 3, t, 2, "split", False))
        k += 1
VID_CASES += [(5, 32, 32, 2, 16, 32, 3, 3, 2, "fp32", False), (5, 32, 64, 1, 16, 16, 3, 1, 2, "winograd", False),
              (5, 100, 100, 3, 16, 32, 3, 3, 2, "split", False),
              (3, 32, 32, 2, 16, 32, 3, 3, 2, "fp32", True), (3, 32, 64, 2, 48, 32, 2, 3, 4, "winograd", False),
              # 256 work-groups per ConvLSTM step in the first launch group (no x-half buffers), 4 in the ragged second
              (3, 64, 128, 1, 16, 16, 130, 2, 128, "fp32", False), (3, 64, 128, 2, 16, 16, 130, 2, 128, "fp32", False),
              (3, 64, 128, 2, 16, 16, 130, 2, 128, "winograd", False)]


@pytest.mark.parametrize("cin,latent,hid,layers,h,w,b,t,chunk,precision,u8", VID_CASES)
def test_video_scoring_workspace(vad, cin, latent, hid, layers, h, w, b, t, chunk, precision, u8):
    m = _vid_model(vad, cin, latent, hid, layers, precision, chunk)
    x = vad.synth.clips(800 + h + w + t, 0, b, t, cin, h, w)
    x = _to_u8(x) if u8 else torch.from_numpy(x).cuda()
    _contract(vad, lambda: m.score_all(x),
              f"video cin {cin} ({latent}, {hid}) x {layers} {h}x{w} b {b} t {t} chunk {chunk} {precision} u8 {u8}")


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("layers,precision", [(1, "fp32"), (2, "winograd")])
def test_video_windows_workspace(vad, stride, layers, precision):
    """Sliding windows: the encoder runs over (chunk - 1) * stride + t source frames, the decoder over chunk * t."""
    m = _vid_model(vad, 3, 32, 64, layers, precision, 2)
    frames = torch.from_numpy(vad.synth.frames(81, 0, 11, 3, 16, 32)).cuda()
    _contract(vad, lambda: m.score_windows(frames, sequence_length=4, stride=stride, errmap=True, recon=True),
              f"windows stride {stride} layers {layers} {precision}")


@pytest.mark.parametrize("latent,hid,layers,precision", [(32, 32, 1, "fp32"), (32, 64, 2, "winograd"), (100, 100, 2, "split")])
def test_video_stateful_workspace(vad, latent, hid, layers, precision):
    """T = 1 continued three times with state_in is state_out; the workspace is sized for this call's T."""
    m = _vid_model(vad, 3, latent, hid, layers, precision, 2)
    x = torch.from_numpy(vad.synth.clips(82, 0, 3, 3, 3, 16, 32)).cuda()

    def call():
        state, res = vad.VideoState.zeros(m, 3, 16, 32, x.device), {}
        for i in range(3):
            o = m.score_stateful(x[:, i:i + 1], state, errmap=True, recon=True)
            assert o["state"] is state
            res[f"step{i}"] = {k: v.clone() for k, v in o.items() if k != "state"}
        res["final"] = state
        return res

    _contract(vad, call, f"stateful ({latent}, {hid}) x {layers} {precision}")


@pytest.mark.parametrize("all_layers", [False, True])
@pytest.mark.parametrize("layers", [1, 2])
def test_convlstm_module_workspace(vad, layers, all_layers):
    """vad_convlstm_seq: with every layer's sequence in the caller's buffer the workspace holds only cell states and z."""
    m = vad.ConvLSTM(input_dim=32, hidden_dims=[32, 40][:layers], kernel_size=3, num_layers=layers, return_all_layers=all_layers)
    load_synthetic(vad, m, 90 + layers)
    m = m.cuda().eval()
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 32, 3, 5)).astype(np.float32)).cuda()
    before = vad.hip.calls["convlstm_seq"]
    _contract(vad, lambda: m(x), f"ConvLSTM layers {layers} all_layers {all_layers}")
    assert vad.hip.calls["convlstm_seq"] == before + 4


# ------------------------------------------------------------------------------ captured graphs
@pytest.mark.parametrize("kind", ["image", "video"])
def test_captured_graph_replays_on_repoisoned_workspace(vad, kind):
    """The workspace pointer is baked into the graph: the arena stays, its contents change between replays."""
    import hip_helpers as H
    if kind == "image":
        m = _img_model(vad, 3, 32, "fp32", 8)
        x = torch.from_numpy(vad.synth.frames(83, 0, 3, 3, 16, 48)).cuda()
        want = dict(scores=True, errmap=True, recon=True, latent=True)
    else:
        m = _vid_model(vad, 3, 32, 64, 2, "fp32", 8)
        x = torch.from_numpy(vad.synth.clips(84, 0, 2, 3, 3, 16, 32)).cuda()
        want = dict(seq=True, frame=True, errmap=True, recon=True)
    with torch.no_grad():
        plain = {k: v.clone() for k, v in m._run_hip(x, **want).items()}
    for k, v in plain.items():
        _finite(k, v, kind)
    pool = H.ArenaPool(0xFF)
    pool.refill = False                          # (a fill issued inside the capture would become a node of the graph)
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        _inject(vad, mp, pool)
        g = m.capture(x, **want)
        assert len(pool.by_size) == 1
        for fill in H.POISONS + (0xFF,):
            pool.poison(fill)
            for v in g.outputs.values():
                v.fill_(NAN)
            out = g.replay()
            pool.check()
            bad = [k for k in plain if not H.same_bits(out[k], plain[k])]
            assert not bad, f"{kind}: replay with fill 0x{fill:02X}: {bad} differ"
        del g


# ------------------------------------------------------------------------------ training steps
def _train_contract(vad, tr, x, label):
    import hip_helpers as H
    running0 = tr.running.clone()

    def call():
        tr.running.copy_(running0)               # (the step updates the running statistics in place)
        loss, recon = tr.forward_backward(x, recon=True)
        return {"loss": loss, "grads": tr.grad.clone(), "running": tr.running.clone(), "recon": recon}

    first = {k: v.clone() for k, v in call().items()}
    again = call()
    torch.cuda.synchronize()
    bad = [k for k in first if not H.same_bits(first[k], again[k])]
    assert not bad, f"{label}: {bad} differ between two plain runs"
    _contract(vad, call, label, plain=first)


VID_TRAIN = [cfg + (prec, 1) for cfg in [(32, 32, 1), (32, 64, 2), (64, 64, 3)]
             for prec in ["fp32", "split", "winograd", "bf16", "bf16_operands"]]      # (latent, hid, layers, precision, wavefront)
VID_TRAIN += [(32, 64, 2, "fp32", 0), (32, 64, 2, "bf16", 0)]                        # the layers strictly one after the other
TRAIN_SHAPES = [(1, 2, 16, 16), (2, 3, 32, 48)]


@pytest.mark.parametrize("latent,hid,layers,precision,wavefront", VID_TRAIN)
def test_video_training_step_workspace(vad, latent, hid, layers, precision, wavefront):
    """Both shapes on one trainer, the smaller first."""
    m = vad.VideoAutoencoder(latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=layers)
    load_synthetic(vad, m, 60 + layers)
    tr = vad.VideoTrainer(m.cuda(), precision=precision)
    l = vad.hip.lib()
    try:
        l.vad_debug_set_lstm_wavefront(wavefront)
        for b, t, h, w in TRAIN_SHAPES:
            x = torch.from_numpy(vad.synth.clips(85, 0, b, t, 3, h, w)).cuda()
            _train_contract(vad, tr, x, f"video step ({latent}, {hid}) x {layers} b {b} t {t} {h}x{w} {precision} wavefront {wavefront}")
    finally:
        l.vad_debug_set_lstm_wavefront(1)


IMG_TRAIN_SHAPES = [(2, 16, 16), (2, 32, 48)]


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd", "bf16_operands"])      # (the precisions ImageTrainer accepts)
@pytest.mark.parametrize("loss", ["mse", "ssim", "combined"])
def test_image_training_step_workspace(vad, loss, precision):
    m = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, m, 66)
    tr = vad.ImageTrainer(m.cuda(), loss=loss, ssim_weight=0.5, window_size=11, precision=precision)
    for n, h, w in IMG_TRAIN_SHAPES:
        x = torch.from_numpy(vad.synth.frames(86, 0, n, 3, h, w)).cuda()
        _train_contract(vad, tr, x, f"image step n {n} {h}x{w} {loss} {precision}")


# ------------------------------------------------------------------------------ criteria and resize through the C ABI
SSIM_SIZES = [(7, 5), (33, 64), (37, 53), (32, 32)]      # 32 x 32 tiles: cut by the edge on one or both axes, and exact


@pytest.mark.parametrize("window", [1, 11, 15])
@pytest.mark.parametrize("size", range(4))
def test_ssim_criterion_workspaces(vad, size, window):
    l = vad.hip.lib()
    h, w = SSIM_SIZES[size]
    for planes in (1, 3):
        _ssim_case(vad, l, planes, h, w, window)


def _ssim_case(vad, l, planes, h, w, window):
    import hip_helpers as H
    rng = np.random.default_rng(100 * h + window + planes)
    pred, target = (H.dev(rng.uniform(-1, 1, (planes, h, w))) for _ in range(2))
    gout = H.dev(np.array([0.75]))
    nf, nb = l.vad_ssim_workspace_floats(planes, h, w), l.vad_ssim_grad_workspace_floats(planes, h, w)
    assert nf == 2 * planes * ((h + 31) // 32) * ((w + 31) // 32) and nb == 3 * planes * h * w

    def run(ws_f, ws_b):
        out3, grad = torch.full((3,), NAN, device="cuda"), torch.full((planes, h, w), NAN, device="cuda")
        vad.hip.check(l.vad_ssim_mse(pred.data_ptr(), target.data_ptr(), planes, h, w, window, 0.5, ws_f.data_ptr(), out3.data_ptr(), H.stream()))
        vad.hip.check(l.vad_ssim_mse_backward(pred.data_ptr(), target.data_ptr(), planes, h, w, window, 0.5, gout.data_ptr(), ws_b.data_ptr(),
                                              grad.data_ptr(), H.stream()))
        torch.cuda.synchronize()
        return {"out3": out3, "grad": grad}

    plain = run(torch.empty(nf, device="cuda"), torch.empty(nb, device="cuda"))
    assert all(bool(torch.isfinite(v).all()) for v in plain.values())
    for fill in H.POISONS:
        pool = H.ArenaPool(fill)
        got = run(pool.new(4 * nf, "vad_ssim_mse workspace").floats(), pool.new(4 * nb, "vad_ssim_mse_backward workspace").floats())
        pool.check()
        bad = [k for k in plain if not H.same_bits(got[k], plain[k])]
        assert not bad, f"ssim planes {planes} {h}x{w} window {window}: {bad} depend on the workspace (fill 0x{fill:02X})"


def _resize_plan(vad, ih, iw, oh, ow):
    l = vad.hip.lib()
    nbytes = l.vad_resize_plan_bytes(ih, iw, oh, ow)
    assert nbytes
    blob = np.empty(nbytes // 4, np.int32)
    vad.hip.check(l.vad_resize_plan(ih, iw, oh, ow, blob.ctypes.data))
    return torch.from_numpy(blob).cuda()


@pytest.mark.parametrize("geo", [(45, 64, 32, 48), (45, 48, 32, 48), (32, 64, 32, 48)])     # both passes, vertical only, horizontal only
def test_resize_workspace(vad, geo):
    import hip_helpers as H
    l = vad.hip.lib()
    ih, iw, oh, ow = geo
    n = 2
    x = torch.from_numpy(np.random.default_rng(ih + iw).integers(0, 256, (n, ih, iw, 3), dtype=np.uint8)).cuda()
    plain = vad.scoring.FrameResizer((oh, ow))(x)
    plan = _resize_plan(vad, ih, iw, oh, ow)
    need = l.vad_resize_workspace_bytes(n, ih, iw, oh, ow)
    both = ih != oh and iw != ow
    assert (need > 0) == both            # at most one pass: no workspace, NULL is accepted
    for fill in H.POISONS:
        arena = H.GuardedArena(need, fill)
        dst = torch.full((n, oh, ow, 3), 0xA5, dtype=torch.uint8, device="cuda")
        vad.hip.check(l.vad_resize_u8(x.data_ptr(), n, ih, iw, 0, plan.data_ptr(), dst.data_ptr(), oh, ow, arena.ptr(), need, H.stream()))
        arena.check("vad_resize_u8 workspace")
        assert torch.equal(dst, plain), f"resize {geo}: the result depends on the workspace (fill 0x{fill:02X})"


# ------------------------------------------------------------------------------ refusals
def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _refused(vad, size, launch, outputs, label):
    """`launch(ws_ptr, ws_bytes)` with one byte less than `size`: VAD_ERR_WS, nothing launched."""
    import hip_helpers as H
    assert size > 1, label
    arena = H.GuardedArena(size, 0x7F)
    before = [o.clone() for o in outputs]
    rc = launch(arena.ptr(), size - 1)
    torch.cuda.synchronize()
    assert rc == ERR_WS, f"{label}: a workspace of size - 1 bytes returned {rc}: {vad.hip.lib().vad_last_error().decode()}"
    for o, b in zip(outputs, before):
        assert H.same_bits(o, b), f"{label}: an output was written by a refused call"
    assert arena.still_poison(), f"{label}: the workspace was written by a refused call"
    arena.check(label)
    assert launch(arena.ptr(), size) == 0, f"{label}: the reported size itself is refused"
    arena.check(label)


def test_refusal_image_score(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    m = _img_model(vad, 3, 32, "fp32", 2)
    b, h, w = 3, 16, 48
    x = torch.from_numpy(vad.synth.frames(1, 0, b, 3, h, w)).cuda()
    packed = m._packed(x.device)
    outs = [_nan(b), _nan(b, h, w), _nan(b, 3, h, w), _nan(b, 32, 1, 3)]
    _refused(vad, l.vad_img_workspace_bytes_c(2, h, w, 32, 3),
             lambda ws, n: l.vad_img_score_c(x.data_ptr(), 0, 0, 3, b, h, w, 32, packed.data_ptr(), ws, n, 2, *[o.data_ptr() for o in outs], st()),
             outs, "vad_img_score_c")


def _vid_refusal_setup(vad):
    m = _vid_model(vad, 3, 32, 64, 2, "fp32", 2)
    return m, m._packed(torch.device("cuda", torch.cuda.current_device()))


def test_refusal_video_score_stateful(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    m, packed = _vid_refusal_setup(vad)
    b, t, h, w = 3, 2, 16, 32
    x = torch.from_numpy(vad.synth.clips(2, 0, b, t, 3, h, w)).cuda()
    state = _nan(l.vad_vid_state_floats(b, h, w, 64, 2))
    outs = [_nan(b), _nan(b, t), _nan(b, t, h, w), _nan(b, t, 3, h, w), state]
    _refused(vad, l.vad_vid_workspace_bytes_c(2, t, h, w, 32, 64, 2, 3),
             lambda ws, n: l.vad_vid_score_s(x.data_ptr(), 0, 0, 3, b, t, h, w, 32, 64, 2, packed.data_ptr(), ws, n, 2,
                                             *[o.data_ptr() for o in outs[:4]], None, state.data_ptr(), st()),
             outs, "vad_vid_score_s")


def test_refusal_video_score_windows(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    m, packed = _vid_refusal_setup(vad)
    f, t, stride, h, w = 9, 4, 3, 16, 32
    nw = l.vad_vid_num_windows(f, t, stride)
    x = torch.from_numpy(vad.synth.frames(3, 0, f, 3, h, w)).cuda()
    outs = [_nan(nw), _nan(nw, t), _nan(nw, t, h, w), _nan(nw, t, 3, h, w)]
    _refused(vad, l.vad_vid_windows_workspace_bytes_c(2, t, stride, h, w, 32, 64, 2, 3),
             lambda ws, n: l.vad_vid_score_windows_c(x.data_ptr(), 0, 0, 3, f, t, stride, h, w, 32, 64, 2, packed.data_ptr(), ws, n, 2,
                                                     *[o.data_ptr() for o in outs], st()),
             outs, "vad_vid_score_windows_c")


def test_refusal_convlstm_seq(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    m = vad.ConvLSTM(input_dim=32, hidden_dims=[32, 40], kernel_size=3, num_layers=2)
    load_synthetic(vad, m, 92)
    m = m.cuda().eval()
    cin_p, hid_p = m._dims()
    packed = m._packed(torch.device("cuda", torch.cuda.current_device()))
    b, t, gh, gw = 2, 3, 3, 5
    x = torch.zeros(b * t * gh * gw * cin_p, device="cuda")
    x.view(b * t * gh * gw, cin_p)[:, :32] = torch.from_numpy(np.random.default_rng(6).standard_normal((b * t * gh * gw, 32)).astype(np.float32)).cuda()
    outs = [_nan(b * t * gh * gw * hid_p), _nan(l.vad_convlstm_state_floats(b, gh, gw, hid_p, 2))]
    _refused(vad, l.vad_convlstm_seq_workspace_bytes(b, t, gh, gw, cin_p, hid_p, 2, 0),
             lambda ws, n: l.vad_convlstm_seq(x.data_ptr(), 0, b, t, gh, gw, cin_p, hid_p, 2, packed.data_ptr(), ws, n, outs[0].data_ptr(), 0,
                                              None, outs[1].data_ptr(), st()),
             outs, "vad_convlstm_seq")


def test_refusal_video_training_step(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    m = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=64, lstm_num_layers=2)
    load_synthetic(vad, m, 62)
    tr = vad.VideoTrainer(m.cuda())
    b, t, h, w = 1, 2, 16, 16
    x = torch.from_numpy(vad.synth.clips(4, 0, b, t, 3, h, w)).cuda()
    tr.grad.fill_(NAN)
    loss, recon = _nan(1), _nan(b, t, 3, h, w)
    _refused(vad, l.vad_vid_train_workspace_bytes(b, t, h, w, 32, 64, 2),
             lambda ws, n: l.vad_vid_train_fwd_bwd(x.data_ptr(), b, t, h, w, 32, 64, 2, tr.flat.data_ptr(), tr.grad.data_ptr(), tr.running.data_ptr(),
                                                   ws, n, 0, loss.data_ptr(), recon.data_ptr(), st()),
             [tr.grad, tr.running, loss, recon], "vad_vid_train_fwd_bwd")


def test_refusal_image_training_step(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    m = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, m, 67)
    tr = vad.ImageTrainer(m.cuda(), loss="combined")
    n_, h, w = 2, 16, 16
    x = torch.from_numpy(vad.synth.frames(5, 0, n_, 3, h, w)).cuda()
    tr.grad.fill_(NAN)
    loss, recon = _nan(1), _nan(n_, 3, h, w)
    _refused(vad, l.vad_img_train_workspace_bytes(n_, h, w, 32),
             lambda ws, n: l.vad_img_train_fwd_bwd(x.data_ptr(), n_, h, w, 32, tr.flat.data_ptr(), tr.grad.data_ptr(), tr.running.data_ptr(), ws, n,
                                                   2, 0.5, 11, 0, loss.data_ptr(), recon.data_ptr(), st()),
             [tr.grad, tr.running, loss, recon], "vad_img_train_fwd_bwd")


def test_refusal_resize(vad):
    l, st = vad.hip.lib(), vad.hip.current_stream
    ih, iw, oh, ow, n_ = 45, 64, 32, 48, 2
    x = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (n_, ih, iw, 3), dtype=np.uint8)).cuda()
    plan = _resize_plan(vad, ih, iw, oh, ow)
    dst = torch.full((n_, oh, ow, 3), 0xA5, dtype=torch.uint8, device="cuda")
    _refused(vad, l.vad_resize_workspace_bytes(n_, ih, iw, oh, ow),
             lambda ws, n: l.vad_resize_u8(x.data_ptr(), n_, ih, iw, 0, plan.data_ptr(), dst.data_ptr(), oh, ow, ws, n, st()),
             [dst], "vad_resize_u8")
