"""Thin numpy <-> libvad_hip.so helpers for the GPU parity tests (layer-level C-ABI calls)."""
import ctypes as C
import importlib

import numpy as np
import torch

hip = importlib.import_module("video-anomaly-detection_amd.hip")

#: arithmetic mode (VAD_PREC_*) the helpers pack and launch with; tests that cover the split mode set it around a case
PRECISION = 0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def nhwc(x_nchw):
    return dev(np.transpose(x_nchw, (0, 2, 3, 1)))


def to_nchw(t_nhwc):
    return t_nhwc.cpu().numpy().transpose(0, 3, 1, 2)


#: what the helpers fill output gaps and guards with (never produced by a kernel: the layers' outputs are O(1))
SENTINEL = -12345.5

#: the two strided layouts of the layer tests: frames `dense + 32 * 7` floats apart (128-byte alignment kept), and step 1 of a
#: `[B][T = 3][dense]` buffer, which is how the ConvLSTM recurrence addresses its operands (offset ti * dense, stride T * dense)
FS_PAD = ("pad", 32 * 7)
FS_TIME = ("time", 3, 1)


class Frames:
    """`n` frames of `shape` (per frame, C-contiguous) inside one flat device buffer.  layout None: dense, and the kernels are
    given frame stride 0; ("pad", k): frames `dense + k` floats apart; ("time", T, ti): frame b is step ti of a [n][T][dense]
    buffer.  Everything outside the frames (gaps, other time steps) holds `fill` and `intact()` says whether it still does."""

    def __init__(self, n, shape, layout=None, fill=float("nan"), data=None):
        dense = int(np.prod(shape))
        if layout is None:
            step, total, off = dense, n * dense, 0
        elif layout[0] == "pad":
            step = dense + layout[1]
            total, off = n * step, 0
        else:
            _, t, ti = layout
            step, total, off = t * dense, n * t * dense, ti * dense
        self.shape, self.fill = (n, *shape), fill
        self.buf = torch.full((total,), fill, device="cuda")
        self.view = self.buf[off:].as_strided((n, dense), (step, 1))
        mask = torch.ones(total, dtype=torch.bool, device="cuda")
        mask[off:].as_strided((n, dense), (step, 1)).fill_(False)
        self.gap = mask
        if data is not None:
            self.view.copy_(data.reshape(n, dense))
        self.ptr = self.buf.data_ptr() + 4 * off
        self.fs = 0 if layout is None else step

    def get(self):
        return self.view.reshape(self.shape)

    def intact(self):
        g = self.buf[self.gap]
        return bool(torch.isnan(g).all()) if self.fill != self.fill else bool((g == self.fill).all())


def _in_frames(x_nchw, layout):
    """NCHW numpy -> NHWC Frames whose gaps are NaN (a read that leaves its frame poisons the result)."""
    t = nhwc(x_nchw)
    return Frames(t.shape[0], tuple(t.shape[1:]), layout, float("nan"), t)


def _out_frames(n, shape, layout):
    """NaN-prefilled output frames; with a layout, the gaps hold SENTINEL."""
    f = Frames(n, shape, layout, SENTINEL)
    f.view.fill_(float("nan"))
    return f


def _result(*outs):
    """Synchronise; every output's gaps must still hold the sentinel; -> NCHW numpy per output."""
    torch.cuda.synchronize()
    for o in outs:
        if not o.intact():
            raise AssertionError("a kernel wrote between the frames of a strided output")
    res = [to_nchw(o.get()) for o in outs]
    return res[0] if len(res) == 1 else tuple(res)


def _bn_ptrs(bn):
    if bn is None:
        return None, None
    arrs = [np.ascontiguousarray(a, np.float32) for a in bn]
    return arrs, (C.c_void_p * 4)(*[a.ctypes.data for a in arrs])


def pack_conv3x3(w, b, bn=None):
    l = hip.lib()
    cout, cin = w.shape[:2]
    w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    keep, bnp = _bn_ptrs(bn)
    if cin == 3:
        wp = np.empty(l.vad_pack_conv3x3_c3_floats(cout), np.float32)
        bo = np.empty(cout, np.float32)
        hip.check(l.vad_pack_conv3x3_c3(w.ctypes.data, b.ctypes.data, bnp, cout, wp.ctypes.data, bo.ctypes.data))
    else:
        wp = np.empty(l.vad_pack_conv3x3_floats(cout, cin), np.float32)
        bo = np.empty(cout, np.float32)
        hip.check(l.vad_pack_conv3x3(w.ctypes.data, b.ctypes.data, bnp, cout, cin, PRECISION, wp.ctypes.data, bo.ctypes.data))
    return dev(wp), dev(bo)


def conv3x3_wino(x_nchw, w, b, bn=None, act=0, pool=False, fs=None):
    """Winograd F(2x2,3x3) form of the same layer (opt-in arithmetic; csrc/conv_wino.hip).  fs: layout of the input AND the
    output frames (see Frames)."""
    l = hip.lib()
    n, cin, h, wd = x_nchw.shape
    cout = w.shape[0]
    w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    keep, bnp = _bn_ptrs(bn)
    wp = np.empty(l.vad_pack_conv3x3_wino_floats(cout, cin), np.float32)
    bo = np.empty(cout, np.float32)
    hip.check(l.vad_pack_conv3x3_wino(w.ctypes.data, b.ctypes.data, bnp, cout, cin, wp.ctypes.data, bo.ctypes.data))
    wp, bo = dev(wp), dev(bo)
    ho, wo = (h // 2, wd // 2) if pool else (h, wd)
    out = _out_frames(n, (ho, wo, cout), fs)
    xin = _in_frames(x_nchw, fs)
    hip.check(l.vad_conv3x3_wino(xin.ptr, xin.fs, wp.data_ptr(), bo.data_ptr(), out.ptr, out.fs, n, h, wd, cin, cout,
                                 act, int(pool), stream()))
    return _result(out)


def convlstm_step_wino(x_nchw, h_nchw, c_nchw, w, b, x_fs=None, h_fs=None, out_fs=None):
    """One ConvLSTMCell step with the gate convolution in Winograd form (h / c None = zero initial state) -> (h', c') NCHW.
    x_fs / h_fs / out_fs: layouts of x, h_prev and h_out (see Frames); c is dense."""
    l = hip.lib()
    n, cx, h, wd = x_nchw.shape
    hid = w.shape[0] // 4
    w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    wp = np.empty(l.vad_pack_conv3x3_wino_floats(4 * hid, cx + hid), np.float32)
    bo = np.empty(4 * hid, np.float32)
    hip.check(l.vad_pack_conv3x3_wino(w.ctypes.data, b.ctypes.data, None, 4 * hid, cx + hid, wp.ctypes.data, bo.ctypes.data))
    wp, bo = dev(wp), dev(bo)
    xin = _in_frames(x_nchw, x_fs)
    hp = _in_frames(h_nchw, h_fs) if h_nchw is not None else None
    cp = nhwc(c_nchw) if c_nchw is not None else None
    ho = _out_frames(n, (h, wd, hid), out_fs)
    co = _out_frames(n, (h, wd, hid), None)
    z = torch.empty(n * h * wd * 4 * hid, device="cuda")
    hip.check(l.vad_convlstm_step_wino(xin.ptr, xin.fs, hp.ptr if hp else None, hp.fs if hp else 0, hip.ptr(cp), wp.data_ptr(),
                                       bo.data_ptr(), ho.ptr, ho.fs, co.ptr, z.data_ptr(), n, h, wd, cx, hid, stream()))
    return _result(ho, co)


def pack_convt(w, b, bn=None):
    l = hip.lib()
    cin, cout = w.shape[:2]
    w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    keep, bnp = _bn_ptrs(bn)
    wp = np.empty(l.vad_pack_convt2x2_floats(cin, cout), np.float32)
    bo = np.empty(cout, np.float32)
    hip.check(l.vad_pack_convt2x2(w.ctypes.data, b.ctypes.data, bnp, cin, cout, PRECISION, wp.ctypes.data, bo.ctypes.data))
    return dev(wp), dev(bo)


def stream():
    return hip.current_stream()


def conv3x3(x_nchw, w, b, bn=None, act=0, pool=False, fs=None):
    """fs: layout of the input AND the output frames (see Frames; the first-layer form takes dense NCHW planes only)."""
    l = hip.lib()
    n, cin, h, wd = x_nchw.shape
    cout = w.shape[0]
    wp, bo = pack_conv3x3(w, b, bn)
    ho, wo = (h // 2, wd // 2) if pool else (h, wd)
    out = _out_frames(n, (ho, wo, cout), fs)
    if cin == 3:
        assert fs is None, "vad_conv3x3_c3 has no frame strides"
        xin = dev(x_nchw)
        hip.check(l.vad_conv3x3_c3(xin.data_ptr(), wp.data_ptr(), bo.data_ptr(), out.ptr, n, h, wd, cout,
                                   act, int(pool), stream()))
    else:
        xin = _in_frames(x_nchw, fs)
        hip.check(l.vad_conv3x3(xin.ptr, xin.fs, wp.data_ptr(), bo.data_ptr(), out.ptr, out.fs, n, h, wd, cin,
                                cout, act, int(pool), PRECISION, stream()))
    return _result(out)


def convt2x2(x_nchw, w, b, bn=None, act=0, fs=None):
    """fs: layout of the input AND the output frames (see Frames)."""
    l = hip.lib()
    n, cin, h, wd = x_nchw.shape
    cout = w.shape[1]
    wp, bo = pack_convt(w, b, bn)
    xin = _in_frames(x_nchw, fs)
    out = _out_frames(n, (2 * h, 2 * wd, cout), fs)
    hip.check(l.vad_convt2x2(xin.ptr, xin.fs, wp.data_ptr(), bo.data_ptr(), out.ptr, out.fs, n, h, wd, cin, cout,
                             act, PRECISION, stream()))
    return _result(out)


def conv1x1(x_nchw, w, b):
    l = hip.lib()
    n, cin, h, wd = x_nchw.shape
    cout = w.shape[0]
    w2 = np.ascontiguousarray(w.reshape(cout, cin), np.float32); b = np.ascontiguousarray(b, np.float32)
    wp = np.empty(l.vad_pack_conv1x1_floats(cout, cin), np.float32)
    bo = np.empty(cout, np.float32)
    hip.check(l.vad_pack_conv1x1(w2.ctypes.data, b.ctypes.data, cout, cin, wp.ctypes.data, bo.ctypes.data))
    wp, bo = dev(wp), dev(bo)
    xin = nhwc(x_nchw)
    out = torch.full((n, h, wd, cout), float("nan"), device="cuda")
    hip.check(l.vad_conv1x1(xin.data_ptr(), wp.data_ptr(), bo.data_ptr(), out.data_ptr(), n * h * wd, cin, cout, stream()))
    torch.cuda.synchronize()
    return to_nchw(out)


def convlstm_step(x, h, c, w, b, x_fs=None, h_fs=None, out_fs=None, alias_c=False):
    """x [N,Cx,H,W], h/c [N,hid,H,W] or None -> (h', c') NCHW numpy.  x_fs / h_fs / out_fs: layouts of x, h_prev and h_out (see
    Frames); c_prev / c_out are dense, and with alias_c the step writes c_out over c_prev."""
    l = hip.lib()
    n, cx, hh, ww = x.shape
    hid = w.shape[0] // 4
    wp, bo = pack_conv3x3(w, b, None)
    xin = _in_frames(x, x_fs)
    hin = _in_frames(h, h_fs) if h is not None else None
    cin_ = nhwc(c) if c is not None else None
    hout = _out_frames(n, (hh, ww, hid), out_fs)
    cout = _out_frames(n, (hh, ww, hid), None)
    if alias_c:
        assert c is not None
        cout.view.copy_(cin_.reshape(n, -1))
        cin_ = cout.get()                                   # (dense layout: a view of the same memory)
        assert cin_.data_ptr() == cout.ptr
    hip.check(l.vad_convlstm_step(xin.ptr, xin.fs, hin.ptr if hin else None, hin.fs if hin else 0, hip.ptr(cin_), wp.data_ptr(),
                                  bo.data_ptr(), hout.ptr, hout.fs, cout.ptr, n, hh, ww, cx, hid, PRECISION, stream()))
    return _result(hout, cout)


def conv3x3_c3_fused(x_nchw, w0, b0, bn0, w1, b1, bn1):
    """Fused enc1 block: conv(3->32)+BN+leaky, conv(32->32)+BN+leaky, maxpool -> NCHW numpy."""
    l = hip.lib()
    n, _, h, wd = x_nchw.shape
    wp0, bo0 = pack_conv3x3(w0, b0, bn0)
    wp1, bo1 = pack_conv3x3(w1, b1, bn1)
    xin = dev(x_nchw)
    out = torch.full((n, h // 2, wd // 2, 32), float("nan"), device="cuda")
    hip.check(l.vad_conv3x3_c3_fused(xin.data_ptr(), wp0.data_ptr(), bo0.data_ptr(), wp1.data_ptr(), bo1.data_ptr(),
                                     out.data_ptr(), n, h, wd, PRECISION, stream()))
    torch.cuda.synchronize()
    return to_nchw(out)


def _guarded(n_floats, guard):
    """NaN-prefilled flat device buffer of n_floats followed by `guard` floats of SENTINEL."""
    t = torch.full((n_floats + guard,), float("nan"), device="cuda")
    t[n_floats:] = SENTINEL
    return t


def _guard_ok(t, n_floats):
    return bool((t[n_floats:] == SENTINEL).all())


def convt2x2_to3_score(x_in, wt, bt, frames, t=0, clip_stride=0, want_recon=True, want_errmap=True):
    """The video scoring tail through the C ABI: x_in [N,32,H,W] NCHW numpy (the decoder's last 32-channel map), wt IOHW
    [32,3,2,2], bt [3], frames [F,3,2H,2W] -> (recon [N,3,2H,2W] | None, errmap [N,2H,2W] | None, partials [N, H, segments]).
    Every output is prefilled with NaN and followed by a guard of two output rows of SENTINEL, which must survive."""
    l = hip.lib()
    n, cin, h, w = x_in.shape
    h2, w2 = 2 * h, 2 * w
    segs = (w + 63) // 64
    nparts = l.vad_score_partials(1, h2, w2)
    assert nparts == h * segs
    guard = 2 * w2
    sizes = {"recon": n * 3 * h2 * w2, "errmap": n * h2 * w2, "partials": n * nparts}
    bufs = {k: _guarded(v, guard) for k, v in sizes.items()}
    xin, wd, bd, xf = nhwc(x_in), dev(wt), dev(bt), dev(frames)
    hip.check(l.vad_convt2x2_to3_score(xin.data_ptr(), wd.data_ptr(), bd.data_ptr(), xf.data_ptr(), bufs["partials"].data_ptr(),
                                       bufs["recon"].data_ptr() if want_recon else None,
                                       bufs["errmap"].data_ptr() if want_errmap else None, n, h, w, cin, t, clip_stride, stream()))
    torch.cuda.synchronize()
    for k, v in sizes.items():
        if not _guard_ok(bufs[k], v):
            raise AssertionError(f"the tail wrote past the end of {k}")
    recon = bufs["recon"][:sizes["recon"]].view(n, 3, h2, w2).cpu().numpy()
    emap = bufs["errmap"][:sizes["errmap"]].view(n, h2, w2).cpu().numpy()
    for name, arr, want in (("recon", recon, want_recon), ("errmap", emap, want_errmap)):
        if not want and not np.isnan(arr).all():
            raise AssertionError(f"the tail wrote {name} although it was given NULL")
    parts = bufs["partials"][:sizes["partials"]].view(n, h, segs).cpu().numpy()
    return recon if want_recon else None, emap if want_errmap else None, parts


def score_finalize(parts, h2, w2, t=1, want_frame=True, want_seq=True):
    """vad_score_finalize on partials [N, nparts] (numpy) -> (frame_scores [N] | None, seq_scores [N / t] | None); outputs
    NaN-prefilled and guarded like those of the tail."""
    l = hip.lib()
    n, nparts = parts.shape
    pd = dev(parts)
    fsb, sqb = _guarded(n, 64), _guarded(n // t, 64)
    hip.check(l.vad_score_finalize(pd.data_ptr(), nparts, n, h2, w2, fsb.data_ptr() if want_frame else None,
                                   sqb.data_ptr() if want_seq else None, t, stream()))
    torch.cuda.synchronize()
    if not (_guard_ok(fsb, n) and _guard_ok(sqb, n // t)):
        raise AssertionError("score_finalize wrote past the end of an output")
    fs, sq = fsb[:n].cpu().numpy(), sqb[:n // t].cpu().numpy()
    if (not want_frame and not np.isnan(fs).all()) or (not want_seq and not np.isnan(sq).all()):
        raise AssertionError("score_finalize wrote an output it was given NULL for")
    return fs if want_frame else None, sq if want_seq else None


# ------------------------------------------------------------------------------ guarded, poisoned workspaces
#: bytes of guard on either side of an arena's body (a multiple of 256: the body keeps the allocation's alignment)
GUARD_BYTES = 1 << 20
GUARD_BYTE = 0xA5
#: dirt this close to a guard's outer end means the stray access may reach beyond memory the test owns
GUARD_EDGE = 4096
#: body fills, the same in every element type: 0x00 = zero ("assumed cleared" hides here), 0xFF = NaN in fp32 and bf16, 0x7F =
#: 3.39e38, the largest finite magnitudes (max / ReLU / max-pool swallow a NaN operand, never a huge finite one)
POISONS = (0x00, 0xFF, 0x7F)


class GuardedArena:
    """One uint8 device allocation `lead | body | tail`: `body` is EXACTLY `nbytes` (what a size function reported, no rounding),
    256-B aligned and filled with `poison`; `lead` and `tail` are GUARD_BYTES of GUARD_BYTE each.  `check()` asserts that
    the guards still hold it: a write before or behind the workspace lands in memory the test owns and is reported."""

    def __init__(self, nbytes, poison=0xFF, device="cuda"):
        self.nbytes = int(nbytes)
        assert self.nbytes >= 0 and GUARD_BYTES % 256 == 0
        self.buf = torch.empty(2 * GUARD_BYTES + self.nbytes, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 256 == 0, "the allocator no longer returns 256-B aligned blocks"
        self.lead = self.buf[:GUARD_BYTES]
        self.body = self.buf[GUARD_BYTES:GUARD_BYTES + self.nbytes]
        self.tail = self.buf[GUARD_BYTES + self.nbytes:]
        self.lead.fill_(GUARD_BYTE)
        self.tail.fill_(GUARD_BYTE)
        self.poison(poison)

    def poison(self, byte):
        self.fill = int(byte)
        self.body.fill_(self.fill)
        return self

    def floats(self):
        """The body as fp32 (nbytes a multiple of 4)."""
        return self.body.view(torch.float32)

    def ptr(self):
        return self.body.data_ptr() if self.nbytes else None

    def still_poison(self):
        """Has nothing written the body since it was filled (a refused call launches nothing)?"""
        torch.cuda.synchronize()
        return bool((self.body == self.fill).all())

    def check(self, what="workspace"):
        torch.cuda.synchronize()
        found = []
        for name, guard in (("lead", self.lead), ("tail", self.tail)):
            dirty = (guard != GUARD_BYTE).nonzero().flatten()
            if dirty.numel() == 0:
                continue
            lo, hi = int(dirty[0]), int(dirty[-1])
            if name == "lead":      # offsets relative to the body's first byte (negative: in front of it)
                msg = f"bytes {lo - GUARD_BYTES}..{hi - GUARD_BYTES} relative to the start of the {self.nbytes}-byte body were written"
                edge = lo < GUARD_EDGE
            else:                   # offsets relative to the body's end (0 = the first byte behind it)
                msg = f"bytes +{lo}..+{hi} behind the end of the {self.nbytes}-byte body were written"
                edge = hi >= GUARD_BYTES - GUARD_EDGE
            if edge:
                msg += f" - the dirt reaches the outer {GUARD_EDGE} bytes of the guard: the overrun may be larger than the guard"
            found.append(f"{what}: {int(dirty.numel())} guard {msg}")
        assert not found, "; ".join(found)


class ArenaPool:
    """The arenas one test hands out: `floats(n)` / `bytes_(n)` make a fresh arena per call (layer tests), `shared(nbytes)` keeps
    ONE arena per distinct size alive (the models' allocation points: a captured graph's workspace pointer stays valid) and fills
    it again on every request unless `refill` is off.  `check()` checks every arena handed out so far."""

    def __init__(self, poison=0xFF):
        self.fill, self.refill = poison, True
        self.arenas, self.by_size = [], {}

    def new(self, nbytes, what="workspace"):
        a = GuardedArena(nbytes, self.fill)
        self.arenas.append((what, a))
        return a

    def floats(self, n):
        return self.new(4 * max(int(n), 1), f"scratch of {int(n)} floats").floats()

    def shared(self, nbytes):
        nbytes = int(nbytes)
        if nbytes not in self.by_size:
            self.by_size[nbytes] = self.new(nbytes, f"workspace of {nbytes} bytes")
        elif self.refill:
            self.by_size[nbytes].poison(self.fill)
        return self.by_size[nbytes].body

    def poison(self, byte):
        self.fill = byte
        for _, a in self.arenas:
            a.poison(byte)

    def check(self):
        for what, a in self.arenas:
            a.check(what)


def same_bits(a, b):
    """Bit identity of two tensors (NaN payloads included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
