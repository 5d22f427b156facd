"""GPU parity of the video scoring tail (vad_convt2x2_to3_score, csrc/tail.hip) and of vad_score_finalize as entry points of
their own, against float64 restatements in numpy, at the shapes where their addressing changes: a partial work-group, rows
shorter than / equal to / longer than one 64-pixel wave segment, a ragged last segment, the sliding-window frame mapping, more
than 256 frames per clip.  The whole-model goldens (32x32 / 64x64 frames) reach none of these."""
import numpy as np
import pytest
import torch

from conftest import load_synthetic, max_abs, rel_err
from oracle import torch_oracle

pytestmark = pytest.mark.gpu

ATOL = 3e-5          # tests/test_hip_layers.py: the bound of the same comparison for the image path's tail (test_dec4_fused_kernel)
SCORE_RTOL = 1e-5    # likewise
TANH_OVERFLOW = 44.4  # exp(2 v) overflows fp32 above this |v|


def _rng(seed):
    return np.random.default_rng(seed)


def _tail_case(rng, n, h, w, nsrc=None, scale=1.0):
    """Inputs as test_hip_layers._dec4_case makes them: post-ReLU activations, weights ~ sqrt(1/32), frames uniform in [-1, 1]
    (every reference score is far from 0).  nsrc: number of source frames when it is not n; scale multiplies weight and bias."""
    x_in = np.maximum(rng.standard_normal((n, 32, h, w)), 0).astype(np.float32)
    wt = (rng.standard_normal((32, 3, 2, 2)) * np.sqrt(1.0 / 32) * scale).astype(np.float32)
    bt = (rng.standard_normal(3) * 0.1 * scale).astype(np.float32)
    frames = rng.uniform(-1, 1, (nsrc or n, 3, 2 * h, 2 * w)).astype(np.float32)
    return x_in, wt, bt, frames


def _tail_ref(x_in, wt, bt, frames, src=None):
    """float64: pre-activations, recon = tanh(ConvTranspose2d k2 s2), channel-mean squared error against frames[src]."""
    n, _, h, w = x_in.shape
    pre = np.einsum("nihw,icab->nchawb", x_in.astype(np.float64), wt.astype(np.float64)).reshape(n, 3, 2 * h, 2 * w)
    pre += bt.astype(np.float64)[None, :, None, None]
    recon = np.tanh(pre)
    x = frames.astype(np.float64)
    emap = ((x[src if src is not None else slice(None)] - recon) ** 2).mean(axis=1)
    return pre, recon, emap


def _segment_sums(emap, h, w):
    """float64 sum of sum_c (x - recon)^2 per (frame, input row, 64-pixel segment): what one partial holds."""
    n = emap.shape[0]
    segs = (w + 63) // 64
    rows = 3.0 * emap.reshape(n, h, 2, 2 * w).sum(axis=2)                       # [n, h, 2w]: both output rows of an input row
    pad = np.zeros((n, h, segs * 128))
    pad[:, :, :2 * w] = rows
    return pad.reshape(n, h, segs, 128).sum(axis=3)


def _check_tail(H, case, ref, t=0, clip_stride=0, label=""):
    """One full call against the float64 reference -> (recon, emap, parts, frame scores); prints the measured maxima."""
    x_in, wt, bt, frames = case
    _, ref_recon, ref_emap = ref
    n, _, h, w = x_in.shape
    recon, emap, parts = H.convt2x2_to3_score(x_in, wt, bt, frames, t, clip_stride)
    assert not np.isnan(recon).any() and not np.isnan(emap).any() and not np.isnan(parts).any()
    assert np.isfinite(recon).all() and np.isfinite(emap).all() and np.abs(recon).max() <= 1.0
    scores, _ = H.score_finalize(parts.reshape(n, -1), 2 * h, 2 * w, 1, True, False)
    ref_scores = ref_emap.mean(axis=(1, 2))
    e_recon, e_emap, e_score = max_abs(recon, ref_recon), max_abs(emap, ref_emap), rel_err(scores, ref_scores)
    print(f"tail {label}: recon {e_recon:.3e} errmap {e_emap:.3e} score rel {e_score:.3e}")
    assert e_recon < ATOL and e_emap < ATOL
    assert e_score < SCORE_RTOL
    # one partial per (row, segment): each against the float64 sum of ITS pixels (every pixel's error map is within ATOL, so a
    # segment of p output pixels is within 3 * ATOL * p), and their sum per frame at the scores' bound
    ref_parts = _segment_sums(ref_emap, h, w)
    npix = np.minimum(64, w - 64 * np.arange(ref_parts.shape[2])) * 4
    assert (np.abs(parts - ref_parts) <= 3 * ATOL * npix[None, None, :]).all()
    assert rel_err(parts.astype(np.float64).sum(axis=(1, 2)), ref_parts.sum(axis=(1, 2))) < SCORE_RTOL
    return recon, emap, parts, scores


@pytest.mark.parametrize("n,h,w", [(3, 1, 1), (1, 3, 8), (2, 4, 64), (2, 5, 72), (1, 2, 136), (5, 3, 20)])
def test_convt2x2_to3_score(n, h, w):
    """ConvTranspose2d(32->3, k2 s2) + Tanh + squared error + per-(row, segment) sums against float64 numpy.  The shapes: a
    single pixel with 3 wave items (a partial work-group), a row shorter than a segment with items % 4 != 0, exactly one segment,
    a ragged second segment (8 valid lanes), three segments, 15 items.  Outputs start as NaN and are followed by a guard; the
    optional outputs may be NULL without changing a bit of the partial sums.
    Measured on MI355X (max over the six shapes): recon 2.7e-07, errmap 3.8e-07, scores 1.4e-07 relative."""
    import hip_helpers as H
    case = _tail_case(_rng(n * 1000 + h * 10 + w), n, h, w)
    x_in, wt, bt, frames = case
    recon, emap, parts, _ = _check_tail(H, case, _tail_ref(*case), label=f"{n}x{h}x{w}")
    for want_recon, want_errmap in ((False, True), (True, False), (False, False)):
        r, e, p = H.convt2x2_to3_score(x_in, wt, bt, frames, 0, 0, want_recon, want_errmap)
        assert np.array_equal(p, parts), (want_recon, want_errmap)
        assert r is None or np.array_equal(r, recon)
        assert e is None or np.array_equal(e, emap)


def test_convt2x2_to3_score_window_mapping():
    """t = 3, clip_stride = 1 over 6 source frames: 12 activation frames = 4 windows, activation frame n scored against source
    frame n // 3 + n % 3 while recon / errmap / partials are indexed by n.  t = 0 and t == clip_stride mean independent clips,
    bit for bit; a window scored alone gives the bits it has inside the batched call."""
    import hip_helpers as H
    rng = _rng(77)
    n, h, w, t = 12, 3, 8, 3
    x_in, wt, bt, frames = _tail_case(rng, n, h, w, nsrc=6)
    src = np.arange(n) // t + np.arange(n) % t
    assert src.max() == 5 and len(set(src)) == 6
    case = (x_in, wt, bt, frames)
    recon, emap, parts, _ = _check_tail(H, case, _tail_ref(x_in, wt, bt, frames, src), t, 1, label="windows")
    for k in range(4):                                                     # window k alone: x offset by k frames
        r, e, p = H.convt2x2_to3_score(x_in[t * k:t * k + t], wt, bt, frames[k:k + t])
        sl = slice(t * k, t * k + t)
        assert np.array_equal(r, recon[sl]) and np.array_equal(e, emap[sl]) and np.array_equal(p, parts[sl]), k
    # independent clips: both spellings, the same bits - and not those of the window mapping
    clips = rng.uniform(-1, 1, (n, 3, 2 * h, 2 * w)).astype(np.float32)
    a = H.convt2x2_to3_score(x_in, wt, bt, clips, 0, 0)
    b = H.convt2x2_to3_score(x_in, wt, bt, clips, t, t)
    ref = _tail_ref(x_in, wt, bt, clips)
    assert max_abs(a[0], ref[1]) < ATOL and max_abs(a[1], ref[2]) < ATOL
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.array_equal(a[0], recon) and not np.array_equal(a[1], emap)   # recon does not depend on the frames, errmap does


def test_convt2x2_to3_score_refusals():
    """Bad arguments are refused before any launch: -1, the matching text, outputs untouched."""
    import hip_helpers as H
    l = H.hip.lib()
    x_in, wt, bt, frames = _tail_case(_rng(3), 2, 2, 4)
    xin, wd, bd, xf = H.nhwc(x_in), H.dev(wt), H.dev(bt), H.dev(frames)
    parts = torch.full((2 * 2,), float("nan"), device="cuda")
    recon = torch.full((2, 3, 4, 8), float("nan"), device="cuda")
    emap = torch.full((2, 4, 8), float("nan"), device="cuda")
    ptrs = [xin.data_ptr(), wd.data_ptr(), bd.data_ptr(), xf.data_ptr(), parts.data_ptr()]

    def call(p=ptrs, cin=32, t=0, stride=0):
        return l.vad_convt2x2_to3_score(*p, recon.data_ptr(), emap.data_ptr(), 2, 2, 4, cin, t, stride, H.stream())

    assert call(cin=64) == -1 and b"cin=64 unsupported" in l.vad_last_error()
    assert call(t=3, stride=0) == -1 and b"bad window mapping" in l.vad_last_error()
    assert call(t=-1, stride=1) == -1 and b"bad window mapping" in l.vad_last_error()
    for i in range(5):
        assert call(p=[None if j == i else q for j, q in enumerate(ptrs)]) == -1 and b"null pointer" in l.vad_last_error(), i
    torch.cuda.synchronize()
    assert torch.isnan(parts).all() and torch.isnan(recon).all() and torch.isnan(emap).all()
    assert call() == 0


def test_convt2x2_to3_score_saturated_tanh():
    """vad_tanh = 1 - 2 * rcp(exp(2 v) + 1) with pre-activations of about +-60 and a share beyond +-44.4, where exp(2 v)
    overflows fp32 (rcp(inf) = 0 -> exactly 1; exp -> 0 -> exactly -1): finite, |recon| <= 1, and the same bounds against
    float64 tanh as everywhere else.  A ragged two-segment map.  (test_hip_layers.test_dec4_tails_saturated_tanh does the same
    for vad_conv3x3_to3_score and vad_dec4_score.)
    Measured on MI355X: recon 2.5e-06, errmap 1.2e-06, scores 2.6e-08 relative."""
    import hip_helpers as H
    case = _tail_case(_rng(1), 2, 5, 72, scale=30.0)
    ref = _tail_ref(*case)
    pre = ref[0]
    assert (pre > TANH_OVERFLOW).mean() > 0.005 and (pre < -TANH_OVERFLOW).mean() > 0.005 and (np.abs(pre) < 1).mean() > 0.01
    assert 60 < np.abs(pre).max() < 120
    assert (ref[1] == 1.0).any() and (ref[1] == -1.0).any()
    recon, _, _, _ = _check_tail(H, case, ref, label="saturated")
    sat = np.abs(pre) > TANH_OVERFLOW
    assert np.array_equal(recon[sat], np.sign(pre[sat]).astype(np.float32))


# (nparts, t, clips): every nparts of {1, 63, 64, 65, 200} and every t of {1, 3, 4, 5, 256, 257, 300} at least once
FINALIZE_CASES = [(1, 1, 3), (63, 3, 3), (64, 4, 1), (65, 5, 3), (200, 256, 1), (200, 257, 3), (64, 300, 3), (65, 257, 1), (63, 1, 1),
                  (200, 4, 3)]
FINALIZE_RTOL = 1e-6


@pytest.mark.parametrize("nparts,t,clips", FINALIZE_CASES)
def test_score_finalize(nparts, t, clips):
    """frame_scores = sum of a frame's partials / (3 * h2 * w2), seq_scores = mean over the t frames of a clip, against float64
    sums: fewer partials than lanes, exactly / just over one lane stripe, several stripes; one frame, frames that do not fill
    the four waves, more than 256 frames (the chunk loop that reuses the shared array).  Either output may be NULL without
    changing the other; a clip finalized alone has the bits it has inside a 3-clip call.
    Measured on MI355X (max over the cases): frame 1.6e-07, seq 4.7e-07, seq against the float64 mean of the
    fp32 frame scores 4.7e-07 (all relative)."""
    import hip_helpers as H
    h2, w2 = 6, 10
    n = clips * t
    parts = _rng(nparts * 1000 + t).uniform(0.25, 4.0, (n, nparts)).astype(np.float32)
    ref_frame = parts.astype(np.float64).sum(axis=1) / (3 * h2 * w2)
    ref_seq = ref_frame.reshape(clips, t).mean(axis=1)
    frame, seq = H.score_finalize(parts, h2, w2, t)
    assert not np.isnan(frame).any() and not np.isnan(seq).any()
    e_frame, e_seq = rel_err(frame, ref_frame), rel_err(seq, ref_seq)
    e_mean = rel_err(seq, frame.astype(np.float64).reshape(clips, t).mean(axis=1))
    print(f"finalize nparts {nparts} t {t} clips {clips}: frame {e_frame:.3e} seq {e_seq:.3e} seq vs mean(frame) {e_mean:.3e}")
    assert e_frame < FINALIZE_RTOL and e_seq < FINALIZE_RTOL and e_mean < FINALIZE_RTOL
    f_only, none = H.score_finalize(parts, h2, w2, t, True, False)
    assert none is None and np.array_equal(f_only, frame)
    none, s_only = H.score_finalize(parts, h2, w2, t, False, True)
    assert none is None and np.array_equal(s_only, seq)
    if clips > 1:
        for c in range(clips):
            f1, s1 = H.score_finalize(parts[c * t:(c + 1) * t], h2, w2, t)
            assert np.array_equal(f1, frame[c * t:(c + 1) * t]) and np.array_equal(s1, seq[c:c + 1]), c


def test_score_finalize_refusals():
    import hip_helpers as H
    l = H.hip.lib()
    parts = torch.ones(6 * 8, device="cuda")
    frame = torch.full((6,), float("nan"), device="cuda")
    seq = torch.full((6,), float("nan"), device="cuda")
    p, f, s = parts.data_ptr(), frame.data_ptr(), seq.data_ptr()
    assert l.vad_score_finalize(p, 8, 6, 4, 4, None, None, 3, H.stream()) == -1 and b"no output requested" in l.vad_last_error()
    assert l.vad_score_finalize(p, 8, 6, 4, 4, f, s, 4, H.stream()) == -1 and b"score_finalize: bad arguments" in l.vad_last_error()
    assert l.vad_score_finalize(p, 8, 6, 4, 4, f, s, 0, H.stream()) == -1 and b"score_finalize: bad arguments" in l.vad_last_error()
    assert l.vad_score_finalize(None, 8, 6, 4, 4, f, s, 3, H.stream()) == -1 and b"score_finalize: bad arguments" in l.vad_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(frame).all() and torch.isnan(seq).all()
    assert l.vad_score_finalize(p, 8, 6, 4, 4, f, s, 3, H.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(frame.cpu(), torch.full((6,), 8.0 / 48.0)) and rel_err(seq[:2].cpu().numpy(), np.full(2, 8.0 / 48.0)) < FINALIZE_RTOL


def test_video_uint8_tail_on_a_ragged_segment(vad):
    """The uint8 form of the tail is reachable through the model only: 2 clips x 2 frames of 32 x 144, so the tail's input map is
    16 x 72 - a full segment and a ragged one of 8 lanes.  uint8 NHWC frames give the bits of the same frames as fp32, and the
    scores are those of the torch oracle."""
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    st = load_synthetic(vad, m, 17)
    m = m.cuda().eval()
    u8 = vad.synth.frames_u8(23, 0, 4, 3, 32, 144, anomalies=True)                   # [N,3,H,W] uint8
    xf = vad.synth.u8_to_unit(u8).reshape(2, 2, 3, 32, 144)
    xu = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).cuda().view(2, 2, 32, 144, 3)
    with torch.no_grad():
        a, b = m.score_all(torch.from_numpy(xf).cuda()), m.score_all(xu)
    for k in ("seq", "frame", "errmap", "recon"):
        assert torch.equal(a[k], b[k]), k
    ref = torch_oracle.vid_scores({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, torch.from_numpy(xf), 32, 1)
    assert rel_err(b["frame"].cpu().numpy(), ref["frame"].numpy()) < SCORE_RTOL
    assert rel_err(b["seq"].cpu().numpy(), ref["seq"].numpy()) < SCORE_RTOL
