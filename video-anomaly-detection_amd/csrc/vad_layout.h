// Packed-weight blob layouts shared by pack.cpp (host packing) and vad_api.hip (launch order).
#pragma once
#include <stddef.h>
#include "vad_hip.h"

int vad_fail(int code, const char* fmt, ...);

// model blob header (4 uint32 words at float offset 0): {VAD_BLOB_MAGIC, tag, dim0, dim1}
constexpr unsigned VAD_BLOB_MAGIC = 0x42444156u;   // "VADB"
constexpr int VAD_BLOB_HEADER_FLOATS = 4;
enum { VAD_BLOB_IMG = 1, VAD_BLOB_VID = 2 };
inline unsigned vad_blob_tag(int kind, int precision) {
    return ((unsigned)VAD_ABI_VERSION << 16) | ((unsigned)precision << 8) | (unsigned)kind;
}

enum { LK_CONV_C3 = 0, LK_CONV, LK_CONVT, LK_TAIL_CONV, LK_LSTM, LK_PROJ, LK_TAIL_CONVT };

struct LayerSlot {
    int kind, cin, cout;
    size_t w, b;   // float offsets into the blob
};
// The reference's constructors take ANY positive latent_dim / lstm_hidden_dim (models/autoencoder.py:161,
// models/video_autoencoder.py:290-296); the kernels tile channels in blocks of 32 (64 hidden channels per ConvLSTM block).
// The packers therefore zero-pad those dimensions: a padded channel has zero weights, zero bias and zero outgoing weights, so
// it carries exactly 0 through LeakyReLU / ReLU / MaxPool and through the ConvLSTM cell (gates 0 -> c' = 0.5*0 + 0.5*0, h' = 0)
// and adds `+ 0*w` terms to the sums it feeds: the results are those of the unpadded network.  Entry points take the REAL
// dimensions; layouts, workspaces and launches use the padded ones below.
inline int vad_pad_up(int x, int m) { return (x + m - 1) / m * m; }
inline int vad_img_latent_p(int latent) { return vad_pad_up(latent, 32); }
// without `proj` (hid == latent) the decoder reads the ConvLSTM output directly: one common padded width
inline int vad_vid_hid_p(int latent, int hid) { (void)latent; return vad_pad_up(hid, 64); }
inline int vad_vid_latent_p(int latent, int hid) { return hid == latent ? vad_pad_up(hid, 64) : vad_pad_up(latent, 32); }

struct ImgLayout {
    LayerSlot layer[16];
    int nlayers;
    int wide;              // in_ch > 3: padded channel count of the input / output planes, else 0
    int latent_p;          // padded latent width (layer[].cin / cout hold padded widths too)
    size_t total;
};
struct VidLayout {
    LayerSlot layer[4 + 8 + 1 + 4];
    int nlayers;
    int wide;              // as in ImgLayout
    int has_proj;          // from the REAL dimensions: lstm_hidden_dim != latent_dim (models/video_autoencoder.py:311-312)
    int latent_p, hid_p;
    size_t total;
};
// in_ch <= 3: the 3-plane path (K = 27 first layer, Cout = 3 tails; 1- and 2-channel models are widened with zero planes by the
// caller).  in_ch > 3 (csrc/wide_io.hip): first and last layer in generic slots of vad_wide_p(in_ch) channels.
constexpr int VAD_MAX_IN_CH = VAD_MAX_IN_CHANNELS;
inline int vad_wide_p(int in_ch) { return vad_pad_up(in_ch, 32); }
ImgLayout img_layout(int in_ch, int latent);            // real dimensions in, padded slots out
VidLayout vid_layout(int in_ch, int latent, int hid, int layers);

// Layer-level ConvLSTM weight set (vad_convlstm_pack / vad_convlstm_seq): per layer a 3x3 slot of (4*hid_p, x + hid_p) in either
// form (direct or Winograd, as in the model blobs) and 4*hid_p biases, each aligned to 4 floats.  vad_seq_slot(.., layers).w is
// the total.
struct VadSeqSlot { size_t w, b; };
inline VadSeqSlot vad_seq_slot(int cin_p, int hid_p, int layer) {
    size_t off = 0;
    VadSeqSlot s{0, 0};
    for (int l = 0; l <= layer; ++l) {
        s.w = off;
        off = (off + vad_pack_conv3x3_wino_floats(4 * hid_p, (l == 0 ? cin_p : hid_p) + hid_p) + 3) & ~(size_t)3;
        s.b = off;
        off = (off + (size_t)4 * hid_p + 3) & ~(size_t)3;
    }
    return s;
}

// ---- resize plan blob (vad_resize_plan, pack.cpp; read by csrc/resize_u8.hip), int32 words:
//   header [16]: {VAD_RESIZE_MAGIC, tag, in_h, in_w, out_h, out_w, kpad_h, kpad_v, off_h, off_v, row0, rows, total words, 0, 0, 0}
//   per axis that is resampled (h = horizontal: in_w -> out_w, v = vertical: in_h -> out_h), at word offset off_*:
//       lo[n_out], count[n_out], (padding to a multiple of 4 words), weights [kpad / 4][n_out][4]
//   weight (g, o, t) = coefficient of tap 4 g + t of output index o, 0 for taps >= count[o]; kpad = the axis' largest count
//   rounded up to a multiple of 4.  An axis whose lengths are equal has no table (kpad 0, off 0): that pass is skipped.
//   row0 / rows: the input rows the vertical pass reads, i.e. the rows the horizontal pass has to produce.
constexpr unsigned VAD_RESIZE_MAGIC = 0x52444156u;   // "VADR"
constexpr int VAD_RESIZE_HEADER_WORDS = 16;
enum { RZ_MAGIC = 0, RZ_TAG, RZ_IN_H, RZ_IN_W, RZ_OUT_H, RZ_OUT_W, RZ_KPAD_H, RZ_KPAD_V, RZ_OFF_H, RZ_OFF_V, RZ_ROW0, RZ_ROWS, RZ_TOTAL };
inline unsigned vad_resize_tag(void) { return ((unsigned)VAD_ABI_VERSION << 16) | 1u; }
constexpr int VAD_RESIZE_MAX_IN = 16384, VAD_RESIZE_MAX_OUT = 4096, VAD_RESIZE_MAX_RATIO = 64;
inline bool vad_resize_axis_ok(int n_in, int n_out) {
    return n_in >= 1 && n_in <= VAD_RESIZE_MAX_IN && n_out >= 1 && n_out <= VAD_RESIZE_MAX_OUT &&
           (long long)n_in <= (long long)VAD_RESIZE_MAX_RATIO * n_out;
}
// taps [lo, hi) of output index o of one axis (pack.cpp; double arithmetic, never contracted)
void vad_resize_bounds(int n_in, int n_out, int o, int* lo, int* hi);
