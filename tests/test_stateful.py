"""Recurrent state carried across calls: `VideoAutoencoder.score_stateful`, `VideoState`, `ConvLSTM.forward(x, hidden_state)` on
the HIP path (vad_vid_score_s, vad_convlstm_seq, vad_state_import / _export).

The exactness statements are the project's usual ones: the step kernels read the same values from another address, so a
clip scored in one call and in pieces with the state carried must give the same BITS.  Comparisons against the reference
(golden vectors, CPU oracle) use the tolerances of tests/test_hip_models.py; no new tolerance is introduced here."""
import ctypes as C
import re
import threading
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_synthetic, max_abs, rel_err
from oracle import torch_oracle
from test_hip_models import ACT_ATOL, SCORE_RTOL

REPO = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["vad_vid_state_floats", "vad_convlstm_state_floats", "vad_vid_score_s", "vad_state_import", "vad_state_export",
               "vad_nchw_to_nhwc_padded", "vad_nhwc_padded_to_nchw", "vad_convlstm_padded_dims", "vad_convlstm_packed_floats",
               "vad_convlstm_pack", "vad_convlstm_seq_workspace_bytes", "vad_convlstm_seq"]


# ------------------------------------------------------------------------------ CPU
def _golden_stack(vad, g, return_all_layers=True):
    m = vad.ConvLSTM(input_dim=32, hidden_dims=[32, 40], kernel_size=3, num_layers=2, return_all_layers=return_all_layers)
    load_synthetic(vad, m, int(g["wseed"]))
    return m.eval()


def _golden_state(g, device="cpu"):
    return [(torch.from_numpy(g[f"h_in{l}"]).to(device), torch.from_numpy(g[f"c_in{l}"]).to(device)) for l in range(2)]


def test_torch_composition_matches_reference_with_initial_state(vad, golden):
    """The torch composition (the checker the GPU tests use where the reference is absent) against the reference's own
    ConvLSTM.forward(x, hidden_state) with a non-zero initial state, in one roll-out and as T = 2 then T = 1."""
    g = golden("stateful/convlstm_state.npz")
    m = _golden_stack(vad, g)
    xs = torch.from_numpy(g["xs"])
    with torch.no_grad():
        outs, finals = m(xs, _golden_state(g))
        outs_a, mid = m(xs[:, :2], _golden_state(g))
        outs_b, finals_b = m(xs[:, 2:], mid)
    for l in range(2):
        assert max_abs(outs[l].numpy(), g[f"seq{l}"]) < ACT_ATOL
        assert max_abs(finals[l][0].numpy(), g[f"h_out{l}"]) < ACT_ATOL and max_abs(finals[l][1].numpy(), g[f"c_out{l}"]) < ACT_ATOL
        assert max_abs(mid[l][0].numpy(), g[f"h_mid{l}"]) < ACT_ATOL and max_abs(mid[l][1].numpy(), g[f"c_mid{l}"]) < ACT_ATOL
        assert max_abs(torch.cat([outs_a[l], outs_b[l]], 1).numpy(), g[f"seq_split{l}"]) < ACT_ATOL
        assert max_abs(finals_b[l][0].numpy(), g[f"h_out_split{l}"]) < ACT_ATOL
        assert max_abs(finals_b[l][1].numpy(), g[f"c_out_split{l}"]) < ACT_ATOL


def test_every_stateful_fixture_has_a_generator():
    """tests/golden/stateful/*.npz are captured from the reference by tests/golden/stateful/make_golden_state.py: every
    committed fixture is one that script regenerates, and vice versa (the rule tests/test_oracle.py holds tests/golden/ to)."""
    import ast
    here = REPO / "tests" / "golden" / "stateful"
    names = set()
    for node in ast.walk(ast.parse((here / "make_golden_state.py").read_text())):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "FIXTURES" for t in node.targets):
            names = {k.value for k in node.value.keys}
    assert names and names == {p.name for p in here.glob("*.npz")}


def test_signatures_bind_every_new_symbol(vad):
    """Every extern "C" symbol the stateful path adds to include/vad_hip.h is bound in hip.SIGNATURES, one for one, and
    exported by the library; the size queries answer 0 for unsupported shapes without a GPU."""
    header = (REPO / "include" / "vad_hip.h").read_text()
    lib = vad.hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/vad_hip.h"
        assert name in vad.hip.SIGNATURES and hasattr(lib, name)
    assert lib.vad_vid_state_floats(2, 32, 48, 40, 3) == 2 * 3 * 2 * 2 * 3 * 64
    assert lib.vad_vid_state_floats(2, 32, 40, 64, 2) == 0 and lib.vad_vid_state_floats(0, 32, 32, 64, 2) == 0
    assert lib.vad_vid_state_floats(1, 32, 32, 64, 9) == 0 and lib.vad_vid_state_floats(1, 32, 32, vad.hip.MAX_WIDTH + 1, 1) == 0
    assert lib.vad_convlstm_state_floats(2, 8, 8, 40, 2) == 0          # the padded width, not the real one
    cin_p, hid_p = C.c_int(), C.c_int()
    assert lib.vad_convlstm_padded_dims(32, (C.c_int * 2)(32, 40), 2, C.byref(cin_p), C.byref(hid_p)) == 0
    assert (cin_p.value, hid_p.value) == (64, 64)
    assert lib.vad_convlstm_padded_dims(48, (C.c_int * 1)(96), 1, C.byref(cin_p), C.byref(hid_p)) == 0
    assert (cin_p.value, hid_p.value) == (64, 128)
    assert "vid_score_stateful" in vad.hip.calls and "convlstm_seq" in vad.hip.calls


def test_stateful_entry_points_refuse_cpu_calls(vad):
    m = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1).eval()
    with torch.no_grad(), pytest.raises(vad.hip.VadError):
        m.score_stateful(torch.zeros(1, 1, 3, 16, 16))                  # no CPU fallback
    with pytest.raises(vad.hip.VadError):
        m.score_stateful(torch.zeros(1, 1, 3, 16, 16))                  # autograd enabled: not an inference call


# ------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def _vid_model(vad, latent, hid, layers, wseed, in_ch=3, precision="fp32"):
    m = vad.VideoAutoencoder(in_channels=in_ch, latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=layers)
    st = load_synthetic(vad, m, wseed)
    m.precision = precision
    return m.cuda().eval(), st


def _clips(vad, seed, b, t, c, h, w, u8=False):
    if u8:
        gen = torch.Generator().manual_seed(seed)
        return torch.randint(0, 256, (b, t, h, w, 3), dtype=torch.uint8, generator=gen).cuda()
    return torch.from_numpy(vad.synth.clips(seed, 0, b, t, c, h, w)).cuda()


@gpu
@pytest.mark.parametrize("all_layers", [False, True])
def test_convlstm_forward_with_state_matches_reference_golden(vad, golden, all_layers):
    g = golden("stateful/convlstm_state.npz")
    m = _golden_stack(vad, g, return_all_layers=all_layers).cuda()
    xs = torch.from_numpy(g["xs"]).cuda()
    before = vad.hip.calls["convlstm_seq"]
    with torch.no_grad():
        outs, finals = m(xs, _golden_state(g, "cuda"))
        outs_a, mid = m(xs[:, :2], _golden_state(g, "cuda"))
        if not all_layers:                 # the reference hands back the last layer's state only: carry the golden's for layer 0
            mid = [(torch.from_numpy(g["h_mid0"]).cuda(), torch.from_numpy(g["c_mid0"]).cuda()), mid]
        outs_b, finals_b = m(xs[:, 2:], mid)
        m.batch_first = False
        outs_t, _ = m(xs.permute(1, 0, 2, 3, 4), _golden_state(g, "cuda"))
    assert vad.hip.calls["convlstm_seq"] == before + 4
    if not all_layers:
        assert isinstance(finals, tuple) and outs.shape == (2, 3, 40, 8, 8)
        outs, finals, outs_a, outs_b, finals_b, outs_t = [outs], [finals], [outs_a], [outs_b], [finals_b], [outs_t]
    for i, l in enumerate(range(2) if all_layers else [1]):
        assert torch.equal(outs_t[i], outs[i])
        assert max_abs(outs[i].cpu().numpy(), g[f"seq{l}"]) < ACT_ATOL
        assert max_abs(finals[i][0].cpu().numpy(), g[f"h_out{l}"]) < ACT_ATOL
        assert max_abs(finals[i][1].cpu().numpy(), g[f"c_out{l}"]) < ACT_ATOL
        assert max_abs(torch.cat([outs_a[i], outs_b[i]], 1).cpu().numpy(), g[f"seq_split{l}"]) < ACT_ATOL
        assert max_abs(finals_b[i][0].cpu().numpy(), g[f"h_out_split{l}"]) < ACT_ATOL
        assert max_abs(finals_b[i][1].cpu().numpy(), g[f"c_out_split{l}"]) < ACT_ATOL


@gpu
@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
def test_zero_state_is_the_stateless_path(vad, precision):
    m, _ = _vid_model(vad, 64, 64, 2, 5, precision=precision)
    x = _clips(vad, 11, 3, 5, 3, 32, 48)
    before = vad.hip.calls["vid_score_stateful"]
    with torch.no_grad():
        want = m.score_all(x)
        frame = m.get_reconstruction_error(x, per_frame=True)
        got = m.score_stateful(x, None, errmap=True, recon=True)
    assert vad.hip.calls["vid_score_stateful"] == before + 1
    assert torch.equal(got["frame"], frame) and torch.equal(got["frame"], want["frame"])
    assert torch.equal(got["errmap"], want["errmap"]) and torch.equal(got["recon"], want["recon"])
    assert isinstance(got["state"], vad.VideoState) and got["state"].key == (3, 32, 48, 64, 2, x.device)


SPLIT_CASES = {
    # name: (in_ch, latent, hid, layers, precision, B, H, W, uint8, chunk)
    "fp32_b1": (3, 64, 64, 2, "fp32", 1, 32, 48, False, None),
    "fp32_b5": (3, 64, 64, 2, "fp32", 5, 64, 64, False, None),
    "split_b5": (3, 64, 64, 2, "split", 5, 32, 48, False, None),
    "split_b1": (3, 64, 64, 2, "split", 1, 64, 64, False, None),
    "winograd_b5": (3, 64, 64, 2, "winograd", 5, 64, 64, False, None),
    "winograd_b1": (3, 64, 64, 2, "winograd", 1, 32, 48, False, None),
    "layers1": (3, 64, 64, 1, "fp32", 5, 32, 48, False, None),
    "layers3": (3, 64, 64, 3, "fp32", 5, 32, 48, False, None),
    "layers3_split": (3, 64, 64, 3, "split", 1, 32, 48, False, None),
    "proj": (3, 48, 96, 2, "fp32", 5, 32, 48, False, None),
    "proj_winograd": (3, 48, 96, 2, "winograd", 1, 64, 64, False, None),
    "width100": (3, 100, 100, 1, "fp32", 5, 32, 48, False, None),
    "in1": (1, 32, 40, 2, "fp32", 5, 32, 48, False, None),
    "in4": (4, 32, 32, 2, "fp32", 5, 32, 48, False, None),
    "in4_split": (4, 32, 32, 2, "split", 1, 64, 64, False, None),
    "uint8": (3, 64, 64, 2, "fp32", 5, 32, 48, True, None),
    "chunked": (3, 64, 64, 2, "fp32", 5, 32, 48, False, 2),
    "chunked_split": (3, 64, 64, 2, "split", 5, 64, 64, False, 2),
}
T_SPLIT = 6
PIECES = [(1,) * T_SPLIT, (3, 1, T_SPLIT - 4), (T_SPLIT - 1, 1)]


@gpu
@pytest.mark.parametrize("case", list(SPLIT_CASES))
def test_splitting_a_call_changes_nothing(vad, case):
    """One call over [B,T] against the same frames in pieces with the state carried - in place and into a fresh state, with
    the ConvLSTM layers strictly in order (wavefront 0) and as a wavefront on helper streams at any size (2): frame scores,
    error maps, reconstructions and the final state blob are bit-identical."""
    in_ch, latent, hid, layers, precision, b, h, w, u8, chunk = SPLIT_CASES[case]
    m, _ = _vid_model(vad, latent, hid, layers, 41, in_ch, precision)
    if chunk:
        m.chunk = chunk
    x = _clips(vad, 12, b, T_SPLIT, in_ch, h, w, u8)
    lib = vad.hip.lib()
    try:
        for wavefront in (0, 2):
            lib.vad_debug_set_lstm_wavefront(wavefront)
            with torch.no_grad():
                whole = m.score_stateful(x, None, errmap=True, recon=True)
                stateless = m.get_reconstruction_error(x, per_frame=True)
            assert torch.equal(whole["frame"], stateless)
            for pieces in PIECES:
                for inplace in (True, False):
                    before = vad.hip.calls["vid_score_stateful"]
                    state, outs, t0 = None, [], 0
                    with torch.no_grad():
                        for n in pieces:
                            prev = state.blob.clone() if state is not None else None
                            o = m.score_stateful(x[:, t0:t0 + n], state, errmap=True, recon=True, inplace=inplace)
                            if state is not None:
                                assert (o["state"] is state) == inplace
                                if not inplace:
                                    assert torch.equal(state.blob, prev)       # the input state is left untouched
                            state = o["state"]
                            outs.append(o)
                            t0 += n
                    assert vad.hip.calls["vid_score_stateful"] == before + len(pieces)
                    what = f"{case}: wavefront {wavefront}, pieces {pieces}, inplace {inplace}"
                    for k in ("frame", "errmap", "recon"):
                        assert torch.equal(torch.cat([o[k] for o in outs], dim=1), whole[k]), f"{what}: {k} differs"
                    assert torch.equal(state.blob, whole["state"].blob), f"{what}: final state differs"
    finally:
        lib.vad_debug_set_lstm_wavefront(1)


@gpu
def test_frame_by_frame_matches_the_oracle_on_one_long_clip(vad):
    """48 frames fed one at a time, B = 2, against the CPU oracle on the same frames as ONE 48-frame clip."""
    m, st = _vid_model(vad, 32, 32, 2, 43)
    x = vad.synth.clips(13, 0, 2, 48, 3, 32, 32)
    xg = torch.from_numpy(x).cuda()
    before = vad.hip.calls["vid_score_stateful"]
    scores, state = vad.scoring.score_frames_stateful(m, (xg[:, t] for t in range(48)), batch=2)
    assert vad.hip.calls["vid_score_stateful"] == before + 48 and scores.shape == (2, 48)
    ref = torch_oracle.vid_scores({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, torch.from_numpy(x), 32, 2)["frame"].numpy()
    err = rel_err(scores, ref)
    print(f"frame-by-frame vs oracle over 48 frames: rel err {err:.3e}")
    assert err < SCORE_RTOL


def _torch_states(vad, model_args, st, x_cpu):
    """(h, c) per layer from the torch composition on the CPU (pinned against the reference by the CPU golden test)."""
    ref = vad.VideoAutoencoder(**model_args)
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    ref.eval()
    ref.convlstm.return_all_layers = True
    with torch.no_grad():
        _, finals = ref.convlstm(ref.encoder(x_cpu))
    return finals


@gpu
@pytest.mark.parametrize("hid,latent", [(64, 64), (40, 32), (100, 100)])
def test_state_conversion(vad, hid, latent):
    args = dict(in_channels=3, latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=2)
    m, st = _vid_model(vad, latent, hid, 2, 44)
    x = vad.synth.clips(14, 0, 3, 4, 3, 32, 48)
    xg = torch.from_numpy(x).cuda()
    state = None
    with torch.no_grad():
        for k in range(4):
            state = m.score_stateful(xg[:, k:k + 1], state)["state"]
            if k in (0, 3):
                want = _torch_states(vad, args, st, torch.from_numpy(x[:, :k + 1]))
                got = state.to_reference()
                assert len(got) == 2
                for l in range(2):
                    assert got[l][0].shape == (3, hid, 2, 3)
                    assert max_abs(got[l][0].cpu().numpy(), want[l][0].numpy()) < ACT_ATOL
                    assert max_abs(got[l][1].cpu().numpy(), want[l][1].numpy()) < ACT_ATOL
    back = vad.VideoState.from_reference(m, state.to_reference())
    assert back.key == state.key and torch.equal(back.blob, state.blob)
    # imported blobs carry exact zeros in the padded channels
    rnd = [(torch.randn(3, hid, 2, 3, device="cuda"), torch.randn(3, hid, 2, 3, device="cuda")) for _ in range(2)]
    imp = vad.VideoState.from_reference(m, rnd)
    planes = imp.blob.view(4, 3, 6, imp.hid_p)
    assert imp.hid_p % 64 == 0 and torch.count_nonzero(planes[..., hid:]) == 0
    assert torch.equal(planes[0, :, :, :hid], rnd[0][0].permute(0, 2, 3, 1).reshape(3, 6, hid))
    for (h1, c1), (h0, c0) in zip(imp.to_reference(), rnd):
        assert torch.equal(h1, h0) and torch.equal(c1, c0)
    clone = state.clone()
    assert clone.blob.data_ptr() != state.blob.data_ptr() and torch.equal(clone.blob, state.blob)


@gpu
def test_streams_are_independent(vad):
    m, _ = _vid_model(vad, 64, 64, 2, 45)
    x = _clips(vad, 15, 4, 5, 3, 32, 48)
    perm = torch.tensor([2, 0, 3, 1], device="cuda")
    with torch.no_grad():
        a = m.score_stateful(x[:, :3])
        b = m.score_stateful(x[perm][:, :3])
        assert torch.equal(b["frame"], a["frame"][perm])
        rows = a["state"].blob.view(4, 4, -1)
        assert torch.equal(b["state"].blob.view(4, 4, -1), rows[:, perm])
        # reset(rows=[1]): stream 1 continues as a fresh stream, the others are untouched
        keep = a["state"].clone()
        s = a["state"].reset(rows=[1])
        assert torch.equal(s.blob.view(4, 4, -1)[:, [0, 2, 3]], keep.blob.view(4, 4, -1)[:, [0, 2, 3]])
        assert torch.count_nonzero(s.blob.view(4, 4, -1)[:, 1]) == 0
        cont = m.score_stateful(x[:, 3:], s)
        fresh = m.score_stateful(x[:, 3:])
        carried = m.score_stateful(x[:, 3:], keep)
    assert torch.equal(cont["frame"][1], fresh["frame"][1])
    assert torch.equal(cont["frame"][[0, 2, 3]], carried["frame"][[0, 2, 3]])
    assert not torch.equal(cont["frame"][1], carried["frame"][1])
    assert torch.equal(cont["state"].blob.view(4, 4, -1)[:, 1], fresh["state"].blob.view(4, 4, -1)[:, 1])
    assert torch.count_nonzero(keep.reset().blob) == 0


@gpu
def test_a_state_that_does_not_fit_is_refused(vad):
    m, _ = _vid_model(vad, 64, 64, 2, 46)
    other, _ = _vid_model(vad, 64, 64, 3, 46)
    x = _clips(vad, 16, 2, 2, 3, 32, 32)
    with torch.no_grad():
        good = m.score_stateful(x)["state"]
        count = dict(vad.hip.calls)
        for bad_x, st in ((_clips(vad, 16, 3, 2, 3, 32, 32), good),                    # another batch size
                          (_clips(vad, 16, 2, 2, 3, 32, 48), good),                    # another frame size
                          (x, other.score_stateful(x)["state"])):                      # another model
            count = dict(vad.hip.calls)
            with pytest.raises(vad.hip.VadError):
                m.score_stateful(bad_x, st)
            assert vad.hip.calls == count                                              # nothing was launched
        with pytest.raises(vad.hip.VadError):
            m.score_stateful(x, good.blob)                                             # a bare tensor is not a state
        with pytest.raises(vad.hip.VadError):
            vad.VideoState(good.blob[:-4], 2, 32, 32, 64, 2)
        with pytest.raises(vad.hip.VadError):
            vad.VideoState(good.blob.cpu().double(), 2, 32, 32, 64, 2)
        with pytest.raises(vad.hip.VadError):
            m.score_stateful(x.cpu(), None)                                            # CPU frames
        with pytest.raises(vad.hip.VadError):
            m.capture(x, state=good)
        # raw ABI: a misaligned blob is refused before anything is launched
        lib = vad.hip.lib()
        packed = m._packed(x.device)
        nbytes = lib.vad_vid_workspace_bytes_c(2, 2, 32, 32, 64, 64, 2, 3)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        frame = torch.full((2, 2), -1.0, device="cuda")
        spare = torch.zeros(good.blob.numel() + 4, device="cuda")
        for sin, sout in ((spare.data_ptr() + 4, None), (None, spare.data_ptr() + 4)):
            rc = lib.vad_vid_score_s(x.data_ptr(), vad.hip.X_F32_NCHW, vad.hip.PREC_FP32, 3, 2, 2, 32, 32, 64, 64, 2, packed.data_ptr(),
                                     ws.data_ptr(), ws.numel(), 2, None, frame.data_ptr(), None, None, sin, sout, vad.hip.current_stream())
            assert rc == -1 and b"aligned" in lib.vad_last_error()
        rc = lib.vad_state_import(spare.data_ptr(), spare.data_ptr(), spare.data_ptr() + 4, 0, 2, 2, 2, 64, 64, 2, vad.hip.current_stream())
        assert rc == -1 and b"aligned" in lib.vad_last_error()
        rc = lib.vad_state_export(spare.data_ptr(), spare.data_ptr(), spare.data_ptr(), 2, 2, 2, 2, 64, 64, 2, vad.hip.current_stream())
        assert rc == -1 and b"layer" in lib.vad_last_error()
        torch.cuda.synchronize()
        assert torch.all(frame == -1.0) and torch.count_nonzero(spare) == 0


@gpu
def test_two_threads_two_states_do_not_interfere(vad):
    """Two threads, two models with different arithmetic, two states on two streams: every round gives bit-for-bit what each
    gives alone (the state is caller-owned; the library shares nothing between them)."""
    ma, _ = _vid_model(vad, 64, 64, 2, 47)
    mb, _ = _vid_model(vad, 64, 64, 2, 47, precision="split")
    x = _clips(vad, 17, 2, 8, 3, 32, 32)

    def run(m):
        state, frames = None, []
        for t in range(8):
            o = m.score_stateful(x[:, t:t + 1], state)
            state = o["state"]
            frames.append(o["frame"])
        return torch.cat(frames, 1), state.blob

    with torch.no_grad():
        want = {"a": run(ma), "b": run(mb)}
    assert not torch.equal(want["a"][0], want["b"][0])
    torch.cuda.synchronize()
    rounds, errors, start = 10, [], threading.Barrier(2)

    def worker(tag, m):
        try:
            stream = torch.cuda.Stream()
            start.wait()
            with torch.no_grad(), torch.cuda.stream(stream):
                for i in range(rounds):
                    frames, blob = run(m)
                    stream.synchronize()
                    if not (torch.equal(frames, want[tag][0]) and torch.equal(blob, want[tag][1])):
                        errors.append(f"{tag}: round {i} differs from the single-threaded result")
                        return
        except Exception as e:                                      # noqa: BLE001 - reported by the main thread
            errors.append(f"{tag}: {e!r}")

    threads = [threading.Thread(target=worker, args=("a", ma)), threading.Thread(target=worker, args=("b", mb))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads) and not errors, errors
