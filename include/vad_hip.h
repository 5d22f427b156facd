/* vad_hip.h — C ABI of libvad_hip.so: the MI355X (gfx950) per-frame anomaly-scoring hot path.
 *
 * The reference (KuldeepChoksi/video-anomaly-detection) has no FFI: its boundary is the Python
 * nn.Module API of models/.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference root).  Everything is plain pointers and sizes; `stream` is a
 * hipStream_t passed as void*.  All device pointers are fp32 unless stated.  Calls are
 * asynchronous on `stream`, never allocate and never synchronise (except vad_prof_read).
 * Every `workspace` / `ws` argument is caller-owned device scratch of the size the matching size function reports: its contents
 * on entry are irrelevant, and no byte outside [ws, ws + size) is read or written.
 *
 * Non-finite data: a NaN (either sign bit) in an input, a state, a weight, a bias or a BatchNorm parameter is never erased - every
 * output whose receptive field holds it is NaN, no other frame's output changes a bit, and scores / losses are non-finite
 * whenever the reference's are (never a silent wrong number).
 *
 * Return value: VAD_OK or a negative VAD_ERR_*; vad_last_error() gives the text.
 */
#ifndef VAD_HIP_H
#define VAD_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VAD_ABI_VERSION 3   /* 2: the arithmetic mode is an argument of every packer / launcher; no process-wide switch.
                             * 3: packed-blob layout of round 3 (tail slot carries the GEMM form the fused dec4 kernel reads, dec4.0 is fp32 in
                             *    every blob, latent / hidden widths zero-padded to the channel tiling): blobs and libraries of ABI 2 are
                             *    rejected by vad_blob_precision and by the device-side tag check */
#define VAD_OK 0
#define VAD_ERR_ARG (-1)   /* bad argument / unsupported shape */
#define VAD_ERR_HIP (-2)   /* HIP runtime error */
#define VAD_ERR_WS (-3)    /* workspace too small */

#define VAD_ACT_NONE 0
#define VAD_ACT_LEAKY 1    /* LeakyReLU(0.2): models/autoencoder.py:41, models/video_autoencoder.py:195 */
#define VAD_ACT_RELU 2     /* ReLU: models/autoencoder.py:106 */

/* Arithmetic of the 3x3 / transposed convolutions.  It is an ARGUMENT (`precision`) of every entry point whose operand
 * layout or kernel depends on it - never process state - so two models with different modes can be scored from two
 * threads at once (the reference's UI calls one global model from worker threads, main.py:50,274).  Weights must be packed
 * and launched with the same value; the model blobs carry it in their header (see vad_img_pack).
 *   VAD_PREC_FP32  exact fp32: v_mfma_f32_32x32x2_f32, bit-for-bit an fp32 fmaf chain (the parity path);
 *   VAD_PREC_SPLIT split fp16: every fp32 operand v is used as hi = fp16(v), lo = fp16((v-hi)*2^11) and a*b is evaluated
 *      as ah*bh + (ah*bl + al*bh)*2^-11 with three v_mfma_f32_32x32x16_f16 and fp32 accumulation.  fp16 products are
 *      exact in fp32, so each product carries 22 significant bits (fp32 has 24); activations and outputs in HBM stay
 *      fp32.  Needs |activation| < 65504.  Opt-in; gated by the same golden-vector and trained-model tests.
 *      Finite range: full accuracy for operand magnitudes in [2^-12, 65520); a finite operand of
 *      65520 or more becomes (Inf, NaN) and every output that reads it NaN - the host packers refuse such a folded weight
 *      with VAD_ERR_ARG, the device-side vad_train_pack_* cannot and write the Inf halves; below 2^-14 an operand is held to
 *      2^-36 absolute (fp16 subnormals are kept), below 2^-36 it is zero. */
#define VAD_PREC_FP32 0
#define VAD_PREC_SPLIT 1
/*   VAD_PREC_BF16  bf16 operands (round to nearest even), one v_mfma_f32_32x32x16_bf16 per 16 channels, fp32 accumulate -
 *      TRAINING ONLY (BASELINE.json configs[4] names bf16): accepted by vad_conv3x3, vad_convt2x2, vad_train_pack_* and the
 *      vad_conv_wgrad and the vad_*_train_fwd_bwd entry points; master weights, BatchNorm, statistics, loss, the first /
 *      last layer and Adam stay fp32 (weight gradients: bf16 operands, fp32 accumulation).
 *      8 significant bits: the scoring entry points and host packers reject it (scores would miss the 1e-4 bar by 60x). */
#define VAD_PREC_BF16 2
/*   VAD_PREC_BF16S bf16 STORAGE as well (training only, the mode `VideoTrainer(precision="bf16")` runs): every activation and
 *      activation-gradient tensor between the kernels - conv outputs before BatchNorm, pooled activations, ConvLSTM operand
 *      and gate buffers, gradient scratch - is bf16 in HBM (half the bytes of the HBM-bound BatchNorm passes, MFMA operands
 *      staged without conversion); arithmetic inside every kernel, BatchNorm statistics (from the fp32 accumulators), cell
 *      states, parameters, parameter gradients, loss and Adam stay fp32.  Layer entry points that take `precision` read /
 *      write bf16 tensors through their `float*` arguments in this mode (element strides stay in elements). */
#define VAD_PREC_BF16S 3
/*   VAD_PREC_WINO  Winograd F(2x2,3x3), scoring only, OPT-IN (`model.precision = "winograd"`): every 3x3 convolution behind
 *                  the first layer computes a 2x2 block of outputs from 16 instead of 36 products per input channel
 *                  (csrc/conv_wino.hip) on the exact-fp32 matrix pipe - all-fp32 arithmetic, but another rounding order than the
 *                  direct form, so NOT bit-identical to VAD_PREC_FP32 (scores differ by ~1e-6 relative; every parity gate
 *                  holds at 1e-5).  Everything else (first layer, transposed convolutions, tails, ConvLSTM cell) is the
 *                  VAD_PREC_FP32 arithmetic.  bench.py's `value` is always VAD_PREC_FP32. */
#define VAD_PREC_WINO 4

int vad_abi_version(void);
const char* vad_last_error(void);   /* per thread */

/* ------------------------------------------------------------------ weight packing (host, CPU)
 * Folds eval-mode BatchNorm2d (eps 1e-5; y = (x-mean)/sqrt(var+eps)*gamma+beta) into the preceding
 * conv in fp64, rounds once to fp32 and re-orders for the kernels' MFMA B-operand loads.
 * bn == NULL means "no BatchNorm after this conv"; bn = {gamma, beta, running_mean, running_var}.
 * With VAD_PREC_SPLIT, vad_pack_conv3x3 / vad_pack_convt2x2 and the model packers built on them (vad_img_pack, vad_vid_pack*,
 * vad_convlstm_pack; these also check the first layer) return VAD_ERR_ARG for a finite FOLDED weight of magnitude >= 65520 - it
 * would be packed as (Inf, NaN) halves; the message names the layer, the element and the value.  A weight that is already
 * NaN / Inf is packed and propagates.  vad_pack_conv3x3_c3 takes no precision (its blob carries both forms) and checks nothing;
 * vad_pack_conv1x1 has no split form.  VAD_PREC_FP32 and VAD_PREC_WINO blobs take every finite value. */

/* Conv2d k3 p1 weight OIHW (Cout,Cin,3,3) -> [9][ceil(Cin/8)][Cout][8]; bias_out[Cout].
 * Replaces nn.Conv2d+nn.BatchNorm2d pairs of models/autoencoder.py:38-79,103-139 and
 * models/video_autoencoder.py:46-52,191-215. */
size_t vad_pack_conv3x3_floats(int cout, int cin);
int vad_pack_conv3x3(const float* w_oihw, const float* bias, const float* const* bn,
                     int cout, int cin, int precision, float* w_packed, float* bias_out);

/* First-layer form (Cin == 3, K = 27 padded to 28): -> [14][2][Cout], followed by the split-fp16 form (both modes). */
size_t vad_pack_conv3x3_c3_floats(int cout);
int vad_pack_conv3x3_c3(const float* w_oihw, const float* bias, const float* const* bn,
                        int cout, float* w_packed, float* bias_out);

/* ConvTranspose2d k2 s2 weight IOHW (Cin,Cout,2,2) -> [4][Cin/8][Cout][8] (quadrant q = 2*a+b).
 * Replaces models/autoencoder.py:104,113,122,131 and models/video_autoencoder.py:244-260. */
size_t vad_pack_convt2x2_floats(int cin, int cout);
int vad_pack_convt2x2(const float* w_iohw, const float* bias, const float* const* bn,
                      int cin, int cout, int precision, float* w_packed, float* bias_out);

/* Conv2d k1 (VideoAutoencoder.proj, models/video_autoencoder.py:311) -> [Cin/8][Cout][8]. */
size_t vad_pack_conv1x1_floats(int cout, int cin);
int vad_pack_conv1x1(const float* w_oihw, const float* bias, int cout, int cin,
                     float* w_packed, float* bias_out);

/* ------------------------------------------------------------------ layer kernels (device)
 * Activations are NHWC fp32.  H, W are the INPUT spatial size.  *_fs = frame stride in floats
 * (0 means dense: H*W*C of that tensor). */

/* x NCHW [N,3,H,W] -> conv3x3(3->Cout)+bias+act(+maxpool2) -> NHWC.  Cout multiple of 32. */
int vad_conv3x3_c3(const float* x_nchw, const float* w_packed, const float* bias, float* out_nhwc,
                   int n, int h, int w, int cout, int act, int pool, void* stream);

/* Fused Encoder.enc1 (models/autoencoder.py:38-46): conv3x3(3->32)+BN+LeakyReLU, conv3x3(32->32)+BN+LeakyReLU,
 * MaxPool2d(2,2) in ONE launch; the 32-channel full-resolution map stays in LDS.  w0/b0 from
 * vad_pack_conv3x3_c3 (cout 32), w1/b1 from vad_pack_conv3x3 (32,32).  out NHWC [N,H/2,W/2,32]. */
int vad_conv3x3_c3_fused(const float* x_nchw, const float* w0, const float* b0, const float* w1, const float* b1,
                         float* out_nhwc, int n, int h, int w, int precision, void* stream);

/* NHWC conv3x3 p1 + bias + act (+ MaxPool2d(2,2) when pool != 0).  Cin multiple of 8 (32 for
 * speed), Cout multiple of 32.  pool needs even H, W. */
int vad_conv3x3(const float* in_nhwc, long long in_fs, const float* w_packed, const float* bias,
                float* out_nhwc, long long out_fs, int n, int h, int w, int cin, int cout,
                int act, int pool, int precision, void* stream);

/* Winograd F(2x2,3x3) form of vad_conv3x3 on the exact-fp32 matrix pipe (csrc/conv_wino.hip): OPT-IN arithmetic - all fp32,
 * 16 instead of 36 multiplies per 2x2 outputs and input channel, NOT bit-identical to vad_conv3x3 (fp32 rounding differs).
 * Same operation as the nn.Conv2d(k3,p1)+BatchNorm2d+activation(+MaxPool2d) pairs of models/autoencoder.py:49-79,103-128.
 * w_packed from vad_pack_conv3x3_wino ([16][Cin/8][Cout][8], U = G g G^T).  Cin, Cout multiples of 32; even H, W. */
size_t vad_pack_conv3x3_wino_floats(int cout, int cin);
int vad_pack_conv3x3_wino(const float* w_oihw, const float* bias, const float* const* bn, int cout, int cin,
                          float* w_packed, float* bias_out);
int vad_conv3x3_wino(const float* in_nhwc, long long in_fs, const float* w_packed, const float* bias,
                     float* out_nhwc, long long out_fs, int n, int h, int w, int cin, int cout,
                     int act, int pool, void* stream);
/* One ConvLSTMCell step (models/video_autoencoder.py:54-85) with the gate convolution in Winograd form: arguments as
 * vad_convlstm_step, w_packed = vad_pack_conv3x3_wino of the (4*hid, cin_x+hid, 3, 3) weight, cin_x == hid, plus
 * z_ws = n*h*w*4*hid floats of scratch for the gate pre-activations (the cell is a second, pointwise launch). */
int vad_convlstm_step_wino(const float* x, long long x_fs, const float* h_prev, long long h_prev_fs, const float* c_prev,
                           const float* w_packed, const float* bias, float* h_out, long long h_out_fs, float* c_out,
                           float* z_ws, int n, int h, int w, int cin_x, int hid, void* stream);

/* NHWC ConvTranspose2d k2 s2 + bias + act: [N,H,W,Cin] -> [N,2H,2W,Cout]. */
int vad_convt2x2(const float* in_nhwc, long long in_fs, const float* w_packed, const float* bias,
                 float* out_nhwc, long long out_fs, int n, int h, int w, int cin, int cout,
                 int act, int precision, void* stream);

/* NHWC 1x1 conv + bias (no activation). */
int vad_conv1x1(const float* in_nhwc, const float* w_packed, const float* bias, float* out_nhwc,
                long long npix, int cin, int cout, void* stream);

/* One ConvLSTMCell step (models/video_autoencoder.py:54-85), gates fused in the conv epilogue.
 * w_packed = vad_pack_conv3x3 of the (4*hid, cin_x+hid, 3, 3) weight.  x [N,H,W,cin_x] (frame
 * stride x_fs), h_prev [N,H,W,hid] (frame stride h_prev_fs), c_prev dense (both NULL mean zeros,
 * models/video_autoencoder.py:87-91).  Writes h_out (frame stride h_out_fs) and c_out (dense;
 * may alias c_prev). */
int vad_convlstm_step(const float* x, long long x_fs, const float* h_prev, long long h_prev_fs,
                      const float* c_prev, const float* w_packed, const float* bias, float* h_out, long long h_out_fs,
                      float* c_out, int n, int h, int w, int cin_x, int hid, int precision, void* stream);

/* Scoring tails.  x is the ORIGINAL input, NCHW [N,3,H2,W2] with H2 = output size.
 * partials: [N][vad_score_partials(H2,W2)] per-tile sums of sum_c (x-recon)^2.
 * recon_nchw (NCHW [N,3,H2,W2]) and errmap ([N,H2,W2], channel mean) may be NULL.
 * Replaces models/autoencoder.py:211-221 and models/video_autoencoder.py:368-384. */
int vad_score_partials(int kind /*0: conv3x3 tail, 1: convT tail*/, int h2, int w2);
/* Conv2d(cin->3) weight OIHW (3,cin,3,3) -> [cin/4][9 taps][4 channels][3 outputs] (per-lane weight rows), followed for
 * cin == 32 by the GEMM form the fused kernel below reads (1024 floats at offset (cin/4)*108: [m = tap*3+co, 32 rows][lane
 * half][16 channel steps]). */
size_t vad_pack_conv3x3_to3_floats(int cin);
int vad_pack_conv3x3_to3(const float* w_oihw, int cin, float* w_packed);
/* Conv2d(32->3) k3 p1 + Tanh (models/autoencoder.py:134-135) on NHWC [N,H2,W2,32]. */
int vad_conv3x3_to3_score(const float* in_nhwc, const float* w_packed /*vad_pack_conv3x3_to3*/,
                          const float* bias3, const float* x_nchw, float* partials,
                          float* recon_nchw, float* errmap, int n, int h2, int w2, int cin,
                          void* stream);
/* dec4 block + scoring in ONE launch: ConvTranspose2d(32->32, k2 s2) + BatchNorm + ReLU, Conv2d(32->3, k3 p1) + Tanh,
 * squared error, channel mean, per-row partial sums (models/autoencoder.py:131-139, 211-221).  in_nhwc [N,H,W,32] is the
 * dec3.3 output; the frame is 2H x 2W; the 32-channel full-resolution map between the two layers is never stored.
 * wt_packed / bt: vad_pack_convt2x2(..., VAD_PREC_FP32) of dec4.0 with dec4.1 folded; w2_gemm: vad_pack_conv3x3_to3's
 * second form; partials: [N][vad_dec4_score_partials(2H, 2W)].  Exact fp32 only. */
int vad_dec4_score_partials(int h2, int w2);
int vad_dec4_score(const float* in_nhwc, const float* wt_packed, const float* bt, const float* w2_gemm,
                   const float* bias3, const float* x_nchw, float* partials, float* recon_nchw, float* errmap,
                   int n, int h, int w, void* stream);
/* ConvTranspose2d(32->3) k2 s2 + Tanh (models/video_autoencoder.py:259-260) on NHWC [N,H,W,32]. */
/* t, clip_stride: activation frame n is scored against x frame (n / t) * clip_stride + n % t (sliding windows
 * over one video); t == 0 or t == clip_stride means frame n (independent clips). */
int vad_convt2x2_to3_score(const float* in_nhwc, const float* w_iohw /*[cin][3][2][2]*/,
                           const float* bias3, const float* x_nchw, float* partials,
                           float* recon_nchw, float* errmap, int n, int h, int w, int cin,
                           int t, int clip_stride, void* stream);
/* frame_scores[N] = sum(partials[n][:]) / (3*H2*W2) in a fixed order (bit-exact under any
 * batching); if seq_scores != NULL also seq_scores[N/t] = mean over t consecutive frames. */
int vad_score_finalize(const float* partials, int nparts, int n, int h2, int w2,
                       float* frame_scores, float* seq_scores, int t, void* stream);

int vad_nhwc_to_nchw(const float* in, float* out, int n, int h, int w, int c, void* stream);
int vad_nchw_to_nhwc(const float* in, float* out, int n, int h, int w, int c, void* stream);

/* ------------------------------------------------------------------ criteria
 * Replaces SSIMLoss.forward (utils/losses.py:51-93) and CombinedLoss.forward (utils/losses.py:114-121) for tensors
 * that need no gradient: pred/target are `planes` = B*C contiguous H x W fp32 planes (NCHW), zero padding
 * window_size/2, Gaussian sigma 1.5, C1 = 1e-4, C2 = 9e-4.  ONE pass over both inputs; no map is materialised.
 * workspace: vad_ssim_workspace_floats(planes,h,w) floats (0 = unsupported shape).
 * out3 (device): { 1 - mean(SSIM), mean((pred-target)^2), (1-alpha)*out3[1] + alpha*out3[0] }. */
size_t vad_ssim_workspace_floats(long long planes, int h, int w);
int vad_ssim_mse(const float* pred, const float* target, long long planes, int h, int w, int window_size,
                 float alpha, float* workspace, float* out3, void* stream);
/* Gradient of out3[2] = (1-alpha)*MSE + alpha*(1 - mean SSIM) with respect to pred (alpha = 1: SSIMLoss, alpha = 0: MSE),
 * times the upstream gradient grad_out (DEVICE scalar, so autograd needs no host synchronisation).  What autograd derives
 * for utils/losses.py:51-121 when train.py:41-46 back-propagates through the criterion.  Two fused passes; workspace:
 * vad_ssim_grad_workspace_floats floats (three adjoint maps). */
size_t vad_ssim_grad_workspace_floats(long long planes, int h, int w);
int vad_ssim_mse_backward(const float* pred, const float* target, long long planes, int h, int w, int window_size,
                          float alpha, const float* grad_out, float* workspace, float* grad_pred, void* stream);
/* Row f-7 - the same criteria as SCORES: one value per frame, and the per-pixel map they are the mean of.
 * recon_nchw: float32 [frames,c,h,w] (a model's reconstruction); x: the original frames, x_format VAD_X_F32_NCHW
 * ([frames,c,h,w] float32) or VAD_X_U8_NHWC ([frames,h,w,3] uint8, c == 3 only, normalised on the load: the bits of the
 * normalised fp32 copy).  Window contract of vad_ssim_mse.  Outputs (device):
 *   ssim_out[f] = 1 - mean over (c,h,w) of the SSIM map of frame f      = SSIMLoss on that frame as a batch of one;
 *   comb_out[f] = (1-alpha)*mse_in[f] + alpha*ssim_out[f]               (NULL, or with mse_in = the frames' squared error);
 *   map_out[f,0,y,x] = mean over c of (1 - SSIM)                        (NULL: no map is written).
 * No atomics; a frame's values do not depend on the other frames of the call.  fp32 whatever mode produced recon.
 * workspace: vad_ssim_score_workspace_floats(frames,h,w) floats (host only; 0 = unsupported shape).  Every argument
 * error is reported before anything is launched. */
size_t vad_ssim_score_workspace_floats(long long frames, int h, int w);
int vad_ssim_score(const float* recon_nchw, const void* x, int x_format, long long frames, int c, int h, int w,
                   int window_size, float alpha, const float* mse_in, float* workspace, float* ssim_out, float* comb_out,
                   float* map_out, void* stream);

/* ------------------------------------------------------------------ training-step kernels
 * The pieces of one optimisation step of train_video.py:44-65 (model.train(); MSELoss; backward; Adam), exact fp32,
 * NHWC activations.  What the reference gets from autograd is stated here as explicit forward/backward kernels.
 * All `ws` arguments are device scratch sized by the matching *_ws_floats function. */

/* Per-channel reductions over an NHWC tensor [npix][c] (c multiple of 4, <= 1024). */
size_t vad_chan_ws_floats(long long npix, int c);
/* Train-mode nn.BatchNorm2d statistics (torch defaults eps 1e-5, momentum 0.1): stats[0..c) = batch mean,
 * stats[c..2c) = 1/sqrt(biased var + eps); running_mean/var (nullable) updated with the unbiased variance. */
int vad_bn_stats(const float* y, long long npix, int c, float eps, float momentum, float* stats,
                 float* running_mean, float* running_var, float* ws, void* stream);
/* out[c] = sum over pixels (bias gradients). */
int vad_chan_sum(const float* g, long long npix, int c, float* out, float* ws, void* stream);
/* BatchNorm(batch stats) + activation (+ MaxPool2d(2,2)) of a conv output y [n,h,w,c]
 * (models/video_autoencoder.py:191-215,242-256 in train mode).  Destination element (frame, pixel, ch) is at
 * out + F*out_fs + pixel*out_ps + ch, with F = frame, or (frame % T)*B + frame / T when remap_t = T > 0 (time-major
 * ConvLSTM operand buffers).  out_fs / out_ps 0 = dense. */
int vad_bn_act_pool_fwd(const float* y, const float* stats, const float* gamma, const float* beta, float* out,
                        long long out_fs, int out_ps, int remap_t, int remap_b, int n, int h, int w, int c,
                        int act, int pool, void* stream);
/* Backward of the above: dout is addressed like `out`.  dy = gradient of the conv output, dense NHWC or (s2d != 0,
 * un-pooled layers) the space-to-depth view [n][h/2][w/2][4][c]; must not alias dout.  dgamma/dbeta [c]; ksums [2c]
 * scratch.  Two passes over y: per-channel sums of the routed gradient, then dy; the routed gradient is never stored. */
int vad_bn_act_pool_bwd(const float* y, const float* stats, const float* gamma, const float* beta, const float* dout,
                        long long dout_fs, int dout_ps, int remap_t, int remap_b, float* dy, int s2d,
                        float* dgamma, float* dbeta, float* ksums, float* ws, int n, int h, int w, int c, int act,
                        int pool, void* stream);
/* ConvLSTMCell gate math (models/video_autoencoder.py:73-83) on pre-activations z [nb*hw][4*hid] (order i,f,g,o): z is
 * overwritten with the activated gates (kept for the backward), c_out = f*c_prev + i*g, h = o*tanh(c_out) written to up
 * to two destinations (frame b, pixel q, channel j) -> h + b*fs + q*ps + j.  c_prev NULL = zeros. */
int vad_lstm_gates_fwd(float* z, const float* c_prev, float* c_out, float* h1, long long h1_fs, int h1_ps,
                       float* h2, long long h2_fs, int h2_ps, int nb, int hw, int hid, void* stream);
/* Backward through the same step: dh = dh1 + dh2 (nullable sources), dc_next nullable -> dz (pre-activation gradients)
 * and dc_prev (may alias dc_next). */
int vad_lstm_gates_bwd(const float* gates, const float* c_prev, const float* c, const float* dh1, long long dh1_fs,
                       int dh1_ps, const float* dh2, long long dh2_fs, int dh2_ps, const float* dc_next, float* dz,
                       float* dc_prev, int nb, int hw, int hid, void* stream);
/* Weight gradient GEMM, K = pixels: a [n,h,w,cin], g [n,h,w,ncols].
 *   taps 9, layout 0: Conv2d k3 p1 weight gradient, dw OIHW (ncols, cin, 3, 3)
 *   taps 1, layout 1: ConvTranspose2d k2 s2 weight gradient from the space-to-depth output gradient
 *                     (ncols = 4*cout, column q*cout+co), dw IOHW (cin, cout, 2, 2)
 *   taps 1, layout 3: ConvTranspose2d(32->3) from the 32-column dpre of vad_convt_to3_mse, dw (32, 3, 2, 2)
 *   taps 1, layout 4: Conv2d k1 (VideoAutoencoder.proj) weight gradient, dw OIHW (ncols, cin, 1, 1) */
size_t vad_conv_wgrad_ws_floats(int n, int h, int taps, int cin, int ncols);
/* precision VAD_PREC_FP32: exact fp32 (v_mfma_f32_32x32x2_f32, two pixels per instruction); VAD_PREC_SPLIT (round 4): both
 * operands split into fp16 (hi, lo) pairs as they are packed, three v_mfma_f32_32x32x16_f16 per 16 pixels (22-bit products, fp32
 * accumulation; |a|, |g| < 65504 and g should sit in the fp16 range - the step scales its gradients, see vad_convt_to3_mse_t);
 * VAD_PREC_BF16: both operands rounded to bf16, v_mfma_f32_32x32x16_bf16 (16 pixels per instruction), fp32 accumulation and
 * fp32 split-K partials. */
int vad_conv_wgrad(const float* a, const float* g, float* dw, float* ws, int n, int h, int w, int cin, int ncols,
                   int taps, int layout, int precision, void* stream);
/* Which kernel form vad_conv_wgrad runs for these arguments under the current vad_debug_set_wgrad_* switches, the partial slots
 * (taps*cin*ncols floats each) it writes into ws and its work items (waves or work-groups).  Host arithmetic only: nothing is
 * launched and no GPU is needed.  VAD_ERR_ARG for arguments vad_conv_wgrad rejects. */
#define VAD_WGRAD_WAVE_F32 0    /* one wave per 32 x 32 tile, exact fp32 (conv_wgrad_kernel) */
#define VAD_WGRAD_WAVE_BF16 1   /* the same tiling on bf16 operands, fp32 or bf16 tensors (conv_wgrad_bf16_kernel) */
#define VAD_WGRAD_WAVE_SPLIT 2  /* the same tiling on split-fp16 operands (conv_wgrad_split_kernel) */
#define VAD_WGRAD_SPLIT_LDS 3   /* split fp16, LDS-staged work-group tiles, 3x3 layers (conv_wgrad_split_lds_kernel) */
#define VAD_WGRAD_RING 4        /* 3x3 layers, every operand row staged once per work-group (conv_wgrad_ring_kernel) */
#define VAD_WGRAD_PAIRS 5       /* bf16 tensors, paired channels, 64 x 64 wave tiles (conv_wgrad_bf16x2_kernel) */
#define VAD_WGRAD_BF16_LDS 6    /* bf16 tensors, LDS-staged work-group tiles (conv_wgrad_bf16_lds_kernel) */
int vad_conv_wgrad_plan(int precision, int n, int h, int w, int cin, int ncols, int taps, int* form, long long* slots,
                        long long* items);
/* First-layer weight gradient: x NCHW [n,3,h,w], g [n,h,w,cout] -> dw OIHW (cout,3,3,3). */
size_t vad_conv_c3_wgrad_ws_floats(int n, int h, int cout);
int vad_conv_c3_wgrad(const float* x_nchw, const float* g, float* dw, float* ws, int n, int h, int w, int cout,
                      void* stream);
/* ConvTranspose2d(32->3,k2,s2)+Tanh+MSELoss(mean), forward and backward in one pass (models/video_autoencoder.py:259-260,
 * train_video.py:54-55): in [n,h,w,32], weight IOHW (32,3,2,2) as stored by torch, x NCHW [n,3,2h,2w].
 * loss[0] = mean((recon-x)^2); recon (NCHW), din [n,h,w,32], dpre32 [n*h*w][32] and dbias3 are optional outputs. */
size_t vad_convt_to3_mse_ws_floats(int n, int h, int w);
int vad_convt_to3_mse(const float* in_nhwc, const float* w_iohw, const float* bias3, const float* x_nchw, float* recon,
                      float* din, float* dpre32, float* loss, float* dbias3, float* ws, int n, int h, int w,
                      void* stream);
/* torch.optim.Adam step (train_video.py:175: weight_decay is L2 added to the gradient) over a flat buffer;
 * grad_scale multiplies g first (1/world_size after a sum all-reduce). */
int vad_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, float grad_scale, void* stream);
/* Device-side operand packing of the CURRENT parameters (no BatchNorm folding in train mode; the layout follows
 * `precision` like the host packers; VAD_PREC_WINO: both operands in Winograd form, vad_pack_conv3x3_wino_floats of room each):
 * fwd = the forward kernels' order (vad_pack_conv3x3 / vad_pack_convt2x2 / vad_pack_conv3x3_c3 layouts);
 * dgrad = the data-gradient operand: for conv3x3 a conv3x3 weight with cin/cout swapped and taps rotated (run it
 * through vad_conv3x3), for convT a 1x1 weight with K = 4*cout (run vad_conv1x1 on the space-to-depth gradient).
 * They never see the values on the host and cannot return an error that depends on them: with VAD_PREC_SPLIT a weight of
 * magnitude >= 65520 is written as (Inf, NaN) halves and every output that reads it is NaN (the host packers refuse it). */
int vad_train_pack_conv3x3(const float* w_oihw, int cout, int cin, float* fwd, float* dgrad, int precision, void* stream);
int vad_train_pack_convt2x2(const float* w_iohw, int cin, int cout, float* fwd, float* dgrad, int precision, void* stream);
int vad_train_pack_conv3x3_c3(const float* w_oihw, int cout, float* fwd, void* stream);
/* Conv2d(cin->3) k3 (ConvAutoencoder's last conv, models/autoencoder.py:134): fwd = vad_pack_conv3x3_to3 layout for the
 * scoring tail kernel; dgrad_c3 = the rotated weights in vad_pack_conv3x3_c3 form (vad_pack_conv3x3_c3_floats(cin) floats):
 * the data gradient is a 3->cin first-layer convolution of the pre-activation gradient. */
int vad_train_pack_conv3x3_to3(const float* w_oihw, int cin, float* fwd, float* dgrad_c3, void* stream);
/* Backward of Conv2d(32->3,k3,p1)+Tanh: recon = tanh(conv(in)) [n,3,h,w]; the upstream gradient is either drecon [n,3,h,w]
 * or (drecon NULL) that of nn.MSELoss against x, times grad_mul (a power of two; 1 = none, see vad_convt_to3_mse_t).  Outputs: dpre scratch [n,3,h,w], din [n,h,w,32], dw (3,32,3,3), db3 [3]. */
size_t vad_conv3x3_to3_bwd_ws_floats(int n, int h, int w, int cin);
int vad_conv3x3_to3_tanh_bwd(const float* in_nhwc, const float* recon, const float* x, const float* drecon,
                             const float* w_dgrad_c3, float* dpre, float* din, float* dw, float* db3, float* ws,
                             int n, int h, int w, int cin, float grad_mul, void* stream);
/* Conv2d k1 (cout, cin, 1, 1): fwd = vad_pack_conv1x1 layout; dgrad = the transposed 1x1 weight (K = cout, N = cin). */
int vad_train_pack_conv1x1(const float* w_oihw, int cout, int cin, float* fwd, float* dgrad, void* stream);

/* bf16-tensor forms of the kernels above (VAD_PREC_BF16S, `VideoTrainer(precision="bf16")`): io16 != 0 means every
 * activation / activation-gradient tensor argument (y, out, dout, dy, z, h1, h2, gates, dh1, dh2, dz, g, in, din, dpre32) is
 * bf16 in memory - strides stay in ELEMENTS - while statistics, cell states, parameters, their gradients and the loss stay
 * fp32; io16 == 0 is the fp32 entry point of the same name without `_t`.  The arithmetic inside is the same fp32 arithmetic
 * on the widened values, results rounded to bf16 (nearest even) where they are stored.  vad_conv3x3 / vad_convt2x2 /
 * vad_conv_wgrad / vad_train_pack_* take precision VAD_PREC_BF16S for the same tensors. */
int vad_chan_sum_t(const void* g, int io16, long long npix, int c, float* out, float* ws, void* stream);
int vad_bn_act_pool_fwd_t(const void* y, int io16, const float* stats, const float* gamma, const float* beta, void* out,
                          long long out_fs, int out_ps, int remap_t, int remap_b, int n, int h, int w, int c, int act, int pool,
                          void* stream);
int vad_bn_act_pool_bwd_t(const void* y, int io16, const float* stats, const float* gamma, const float* beta, const void* dout,
                          long long dout_fs, int dout_ps, int remap_t, int remap_b, void* dy, int s2d, float* dgamma, float* dbeta,
                          float* ksums, float* ws, int n, int h, int w, int c, int act, int pool, void* stream);
int vad_lstm_gates_fwd_t(void* z, int io16, const float* c_prev, float* c_out, void* h1, long long h1_fs, int h1_ps,
                         void* h2, long long h2_fs, int h2_ps, int nb, int hw, int hid, void* stream);
int vad_lstm_gates_bwd_t(const void* gates, int io16, const float* c_prev, const float* c, const void* dh1, long long dh1_fs,
                         int dh1_ps, const void* dh2, long long dh2_fs, int dh2_ps, const float* dc_next, void* dz,
                         float* dc_prev, int nb, int hw, int hid, void* stream);
/* Routed first-layer weight gradient of the bf16-tensor step (round 4; csrc/wgrad.hip conv_c3_wgrad_routed_kernel): BatchNorm's
 * backward pass A with `codes` != NULL writes one routing byte per pooled element (argmax position | sign << 2) instead of running
 * pass B; vad_conv_c3_wgrad_routed then forms dW of Conv2d(3 -> 32) + BatchNorm + LeakyReLU + MaxPool2 from the POOLED gradient
 * d(out) ([n, h/2, w/2, 32]: bf16 with io16, bf16 MFMAs throughout; else fp32, T1 on the exact-fp32 MFMA and S in split-fp16), the codes, the input planes and the layer's own weights / statistics (dW = sc (T1 - k1 SX - k2
 * invstd ((W S) + (b - mean) SX)), S the Gram matrix of the input patches) - the dense conv-output gradient is never formed. */
int vad_bn_act_pool_bwd_codes_t(const void* y, int io16, const float* stats, const float* gamma, const float* beta, const void* dout,
                                long long dout_fs, int dout_ps, int remap_t, int remap_b, void* dy, int s2d, float* dgamma,
                                float* dbeta, float* ksums, float* ws, int n, int h, int w, int c, int act, int pool,
                                unsigned char* codes, void* stream);
size_t vad_conv_c3_wgrad_routed_ws_floats(int n, int h);
int vad_conv_c3_wgrad_routed_ok(int h, int w, int cout);
int vad_conv_c3_wgrad_routed(const float* x_nchw, const void* dout, int io16, const unsigned char* codes, const float* w0, const float* b0,
                             const float* stats, const float* gamma, const float* ksums, float* dw, float* ws, int n, int h, int w,
                             int cout, void* stream);
int vad_debug_set_c3_routed(int on);     /* A/B: 0 = pass B + vad_conv_c3_wgrad_t (rounds 1-3); default 1 */
int vad_c3_routed_enabled(void);
int vad_conv_c3_wgrad_t(const float* x_nchw, const void* g, int io16, float* dw, float* ws, int n, int h, int w, int cout,
                        void* stream);
/* grad_mul (a power of two, 1 = none) multiplies every gradient this call emits (din, dpre32, dbias3), not the loss: the
 * split-fp16 training step runs its whole backward on gradients scaled into the fp16 range and unscales the parameter
 * gradients at the end (vad_scale_floats) - exact in fp32 either way. */
int vad_convt_to3_mse_t(const void* in_nhwc, int io16, const float* w_iohw, const float* bias3, const float* x_nchw, float* recon,
                        void* din, void* dpre32, float* loss, float* dbias3, float* ws, int n, int h, int w, float grad_mul,
                        void* stream);
/* The same layer as separate launches, for a criterion evaluated between them (SSIMLoss / CombinedLoss need the whole
 * reconstruction before any gradient exists).  io16 != 0: in / din / dpre32 are bf16, everything else fp32.
 *   fwd: recon [n,3,2h,2w] = tanh(convT(in) + bias), the bits vad_convt_to3_mse_t writes for the same input.
 *   bwd: from recon and drecon = d loss / d recon (both NCHW fp32; the layer's input is not read): dpre32 [n*h*w][32]
 *        (column q*3+c = grad_mul * drecon * (1 - recon^2), columns 12..31 zero), din [n,h,w,32] (nullable) and dbias3
 *        (nullable; needs ws of vad_convt_to3_tanh_bwd_ws_floats floats).  grad_mul: a power of two, as above. */
size_t vad_convt_to3_tanh_bwd_ws_floats(int n, int h, int w);
int vad_convt_to3_tanh_fwd_t(const void* in_nhwc, int io16, const float* w_iohw, const float* bias3, float* recon, int n, int h, int w,
                             void* stream);
int vad_convt_to3_tanh_bwd_t(const float* recon, const float* drecon, const float* w_iohw, void* din, void* dpre32, int io16,
                             float* dbias3, float* ws, int n, int h, int w, float grad_mul, void* stream);
/* p[i] *= mul, i < n. */
int vad_scale_floats(float* p, long long n, float mul, void* stream);
/* Conv2d k1 with `precision`: VAD_PREC_BF16S = bf16 tensors and bf16 operands (weights from vad_train_pack_conv1x1_p with the
 * same precision), anything else = vad_conv1x1 / vad_train_pack_conv1x1. */
int vad_train_pack_conv1x1_p(const float* w_oihw, int cout, int cin, float* fwd, float* dgrad, int precision, void* stream);
int vad_conv1x1_p(const void* in, const float* w_packed, const float* bias, void* out, long long npix, int cin, int cout,
                  int precision, void* stream);
/* First layer (x NCHW fp32 [N,3,H,W]) -> conv3x3(3->Cout) + bias, un-activated, into a bf16 NHWC tensor. */
int vad_conv3x3_c3_bf16(const float* x_nchw, const float* w_packed, const float* bias, void* out_bf16, int n, int h, int w,
                        int cout, void* stream);
/* ... with bf16 MFMA OPERANDS as well (input taps and weights rounded to bf16, nearest even; K = 27 -> 32 = two
 * v_mfma_f32_32x32x16_bf16 per 32 pixels; fp32 accumulation from the bias): what the VAD_PREC_BF16S training step runs. */
int vad_conv3x3_c3_bf16op(const float* x_nchw, const float* w_packed, const float* bias, void* out_bf16, int n, int h, int w,
                          int cout, void* stream);

/* ------------------------------------------------------------------ whole training step (row f-1)
 * Replaces the loop body of train_video.py:50-60 for VideoAutoencoder(in_channels=3, latent_dim, lstm_hidden_dim,
 * lstm_num_layers) (both dims multiples of 32, hidden <= 256; `proj` is the 1x1 conv when they differ): train-mode forward (batch-statistics BatchNorm, running stats updated when `running`
 * is given), nn.MSELoss, and the full backward.  precision VAD_PREC_FP32: exact fp32; VAD_PREC_SPLIT / VAD_PREC_BF16: the 3x3
 * and transposed convolutions (forward + data gradients) use split-fp16 / bf16 operands with fp32 accumulation (bf16: the
 * weight gradients too), the rest (first and last layer, 1x1 data gradients, BatchNorm, gates, loss, Adam, master weights;
 * in split mode also the weight gradients) stays fp32.  VAD_PREC_BF16S: VAD_PREC_BF16 with every activation / gradient tensor
 * of the workspace stored as bf16.  VAD_PREC_WINO: fp32 everywhere, the 3x3 convolutions behind the first layer (forward + data
 * gradients, ConvLSTM gate convolutions included) as Winograd F(2x2,3x3) (csrc/conv_wino.hip).  With more than one ConvLSTM layer
 * and a small batch the layers run as a wavefront on library-owned helper streams, and the weight-gradient GEMMs run on a helper
 * stream beside the BatchNorm / data-gradient chain; both fork from and join `stream` (vad_debug_set_lstm_wavefront(0): serial
 * order, bit-identical).  params / grads: flat fp32 device buffers of vad_vid_train_nparams
 * floats, torch layouts in named_parameters() order (see csrc/train_step.hip); running: vad_vid_train_nstats floats,
 * {running_mean, running_var} per BatchNorm in module order.  x [B,T,3,H,W]; loss: device float[1];
 * recon (nullable) [B,T,3,H,W].  Every gradient is overwritten (no accumulation), so there is no zero_grad.
 * Follow with vad_adam_step on the same flat buffers (after the gradient all-reduce when data-parallel). */
size_t vad_vid_train_nparams(int latent, int hid, int layers);
size_t vad_vid_train_nstats(int latent, int hid, int layers);
size_t vad_vid_train_workspace_bytes(int b, int t, int h, int w, int latent, int hid, int layers);
/* Debug: float offsets of the saved forward buffers inside the training workspace (order documented at the definition in
 * csrc/train_step.hip); returns the number of entries written to out[cap] or a negative VAD_ERR_*. */
/* debug: record the branch decisions (pooling argmax, activation sign) of the following vad_bn_act_pool_bwd calls, one byte
 * per output pixel and channel, consecutively into buf; (NULL, 0) stops.  See csrc/train_ops.hip. */
int vad_debug_set_train_decisions(void* buf, size_t bytes);
size_t vad_debug_train_decisions_used(void);
/* A/B: 0 = the weight gradients of the bf16-tensor mode use the one-channel-per-lane kernel everywhere; 1 = the paired-channel
 * kernel (dword loads, 64 x 64 wave tiles) where cin and ncols are multiples of 64; 2 = its LDS-staged work-group
 * form where ncols is a multiple of 128; 3 (default) = the row-ring kernel for the 3x3 layers with ncols % 64 == 0 and cin % 64 == 0
 * or cin == 32 (every operand row staged once per work-group, csrc/wgrad.hip), 2 elsewhere. */
int vad_debug_set_wgrad_pairs(int on);
/* A/B: 0 = VAD_PREC_SPLIT weight gradients on the exact-fp32 kernel (rounds 2-3); 1 = the per-lane split-fp16 kernel; 2 = its
 * LDS-staged form for the 3x3 layers it takes; 3 (default) = the row-ring kernel for those layers. */
int vad_debug_set_wgrad_split(int on);
/* A/B: 0 = exact-fp32 3x3 weight gradients on the per-wave kernel (rounds 1-3); 1 (default) = the row-ring kernel where it applies. */
int vad_debug_set_wgrad_ring_f32(int on);
/* 1 (default): the BatchNorm forward / backward-apply passes on bf16 tensors take eight channels per thread (16-byte accesses);
 * 0: four, like the fp32 form.  Identical results (every element goes through the same expressions). */
int vad_debug_set_bn_wide(int on);
/* debug / A-B: 0 = the split-fp16 training steps run their backward on unscaled gradients (round 3's form: operands below the
 * fp16 range at large batches); default 1 = scaled by a power of two and unscaled at the end (csrc/train_step.hip). */
int vad_debug_set_split_grad_scale(int on);
int vad_split_grad_scale_enabled(void);
/* debug: return from vad_vid_train_fwd_bwd(_l) early with the gradient scratch intact.  20 = after the last layer and the
 * criterion; 2, 1, 0 = after the backward of decoder stage j; 10 + l = after the backward of ConvLSTM layer l; 30 + k = after the
 * backward of encoder stage k; -1 (default) = the whole step.  Every stop runs without the weight-gradient helper stream, stops
 * >= 10 also without the layer wavefront (bit-identical orders).  What g0 / g2 hold at each stop: csrc/train_step.hip. */
int vad_debug_set_train_stop(int stage);
int vad_vid_train_debug_layout(int b, int t, int h, int w, int latent, int hid, int layers, long long* out, int cap);
/* debug: the offsets vad_vid_train_debug_layout leaves out, for the criterion loss_kind: pseq (0 without proj), dcat[l], dzl[l],
 * dc[l], recon, drecon (both 0 with loss_kind 0), ksums (k1 / k2 of the last BatchNorm backward), ws_floats.  Same return
 * convention. */
int vad_vid_train_debug_layout2(int b, int t, int h, int w, int latent, int hid, int layers, int loss_kind, long long* out, int cap);
int vad_vid_train_fwd_bwd(const float* x, int b, int t, int h, int w, int latent, int hid, int layers,
                          const float* params, float* grads, float* running, void* workspace, size_t workspace_bytes,
                          int precision, float* loss, float* recon, void* stream);
/* The same step with the criterion as an argument (`_l`): loss_kind 0 = nn.MSELoss - exactly the two entry points above, which
 * are these with loss_kind 0 -, 1 = SSIMLoss(window_size), 2 = CombinedLoss(alpha, window_size), on the frames of the batch as one
 * [B*T,3,H,W] batch (the one way SSIMLoss takes clips, as in scoring.validate).  Kinds 1 / 2 run the last layer as
 * vad_convt_to3_tanh_fwd_t, vad_ssim_mse, vad_ssim_mse_backward, vad_convt_to3_tanh_bwd_t; the criterion is fp32 in every
 * precision mode.  The workspace of kinds 1 / 2 is that of kind 0 plus, behind it, recon, d recon and the criterion's scratch;
 * 0 = unsupported shape or loss_kind. */
size_t vad_vid_train_workspace_bytes_l(int b, int t, int h, int w, int latent, int hid, int layers, int loss_kind);
int vad_vid_train_fwd_bwd_l(const float* x, int b, int t, int h, int w, int latent, int hid, int layers,
                            const float* params, float* grads, float* running, void* workspace, size_t workspace_bytes,
                            int loss_kind, float alpha, int window_size, int precision, float* loss, float* recon, void* stream);

/* Image autoencoder counterpart (train.py:28-52; not a SURVEY section 8 row): ConvAutoencoder(in_channels=3, latent_dim), x
 * [N,3,H,W]; loss_kind 0 = nn.MSELoss (train.py default), 1 = SSIMLoss(window_size), 2 = CombinedLoss(alpha, window_size)
 * (train.py:149-158).  Same flat-buffer conventions and arithmetic modes as the video step. */
size_t vad_img_train_nparams(int latent);
size_t vad_img_train_nstats(int latent);
size_t vad_img_train_workspace_bytes(int n, int h, int w, int latent);
int vad_img_train_fwd_bwd(const float* x, int n, int h, int w, int latent, const float* params, float* grads,
                          float* running, void* workspace, size_t workspace_bytes, int loss_kind, float alpha,
                          int window_size, int precision, float* loss, float* recon, void* stream);

/* Synthetic frames on device, bit-identical to synth.frames() (numpy): NCHW fp32 in [-1,1].  anomalies: 0 = none,
 * 1 = labelled frames carry a saturated 32 x 32 patch, k >= 2 = a k x k patch. */
int vad_synth_frames(float* out_nchw, unsigned long long seed, long long first_frame, long long n,
                     int c, int h, int w, int anomalies, void* stream);

/* ------------------------------------------------------------------ whole-model scoring
 * Image autoencoder.  Replaces ConvAutoencoder.forward / get_latent / get_reconstruction_error
 * (models/autoencoder.py:181-221) as driven by evaluate.compute_auroc (evaluate.py:56-64).
 * params: VAD_IMG_NPARAMS host pointers in state_dict order with num_batches_tracked removed. */
#define VAD_IMG_NPARAMS 92
/* latent_dim / lstm_hidden_dim: ANY value in [1, VAD_MAX_WIDTH], as the reference's constructors take
 * (models/autoencoder.py:161, models/video_autoencoder.py:290-296; train_video.py:304-326 exposes them as flags).  The
 * kernels tile channels by 32 (64 hidden channels per ConvLSTM block); the packers zero-pad other widths (zero weights and
 * bias in, zero weights out: a padded channel stays exactly 0 through every layer, results are those of the unpadded
 * network).  Every entry point takes the REAL dimensions. */
#define VAD_MAX_WIDTH 4096
/* Frame sizes: H and W positive multiples of 16 (four 2x2 poolings) with H * W <= VAD_MAX_FRAME_PIXELS = 2^23 - 1.  The kernels
 * multiply pixel indices as 24-bit operands (4K UHD, 8,294,400 pixels, fits).  Every scoring and training entry point refuses a
 * larger frame with VAD_ERR_ARG before anything is launched and every *_workspace_bytes query answers 0 for it; the layer entry
 * points (vad_conv3x3*, vad_convlstm_step*, vad_convt2x2, vad_dec4_score) hold the same limit for their own h x w maps, next to
 * the byte limit of 2^31 bytes per frame of any of their tensors. */
#define VAD_MAX_FRAME_PIXELS 8388607
/* The packed blob starts with a 16-byte header {magic "VADB", tag = abi<<16 | precision<<8 | model kind, dims}; the
 * layers follow.  Pack with the precision the blob will be launched with: the kernel that finalises the scores compares
 * the tag with the launch's `precision` on the device and returns NaN scores on a mismatch (never a silent wrong number).
 * vad_blob_precision reads the mode back from a HOST copy of a blob (negative VAD_ERR_ARG if it is not one). */
size_t vad_img_packed_floats(int in_ch, int latent);
int vad_img_pack(const float* const* params, int nparams, int in_ch, int latent, int precision, float* packed_host);
int vad_blob_precision(const float* packed_host);
size_t vad_img_workspace_bytes(int chunk, int h, int w, int latent);
/* x NCHW [B,3,H,W] on device.  Frames are processed in chunks of `chunk` through `workspace`.
 * Outputs (device, any may be NULL): scores [B]; errmap [B,H,W]; recon NCHW [B,3,H,W];
 * latent NCHW [B,latent,H/16,W/16].  This short form is float input + VAD_PREC_FP32 (blob packed likewise);
 * vad_img_score_x takes the input format and the arithmetic mode. */
int vad_img_score(const float* x_nchw, long long b, int h, int w, int latent,
                  const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk,
                  float* scores, float* errmap, float* recon_nchw, float* latent_nchw, void* stream);

/* Video ConvLSTM autoencoder.  Replaces VideoAutoencoder.forward / get_reconstruction_error
 * (models/video_autoencoder.py:329-384) as driven by evaluate_video.py:138-154,346-352.
 * params: host pointers in state_dict order with num_batches_tracked removed:
 *   4 x (conv w,b, bn g,b,m,v) ; layers x (cell w,b) ; [proj w,b] ; 3 x (convT w,b, bn g,b,m,v) ; convT w,b */
int vad_vid_nparams(int layers, int has_proj);
size_t vad_vid_packed_floats(int latent, int hid, int layers);
int vad_vid_pack(const float* const* params, int nparams, int latent, int hid, int layers, int precision, float* packed_host);
size_t vad_vid_workspace_bytes(int chunk_clips, int t, int h, int w, int latent, int hid, int layers);
/* x [B,T,3,H,W].  Outputs (any may be NULL): seq_scores [B]; frame_scores [B,T];
 * errmap [B,T,H,W]; recon [B,T,3,H,W].  Asynchronous on `stream`; launch groups smaller than one work-group per CU run the
 * ConvLSTM layers as a wavefront on library-owned helper streams that fork from and join `stream` (vad_debug_set_lstm_wavefront). */
int vad_vid_score(const float* x, long long b, int t, int h, int w, int latent, int hid, int layers,
                  const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk_clips,
                  float* seq_scores, float* frame_scores, float* errmap, float* recon, void* stream);

/* Developer switches for A/B timing in one process (process-wide, debug only; the library never writes them itself).
 * Bit 0: 1 = persistent work-groups with register prefetch of the next stage (default), 0 = one tile per work-group
 * (bit-identical results).  Bit 1: pricing runs whose results are NOT valid - exact kernels drop their epilogue stores,
 * split kernels read no weights.  Bit 2: alternative cout-64 tiling.  Bit 3: never use the small-grid (16x16x4) ConvLSTM
 * kernel, bit 4: always use it, bit 5: never compute the ConvLSTM x halves ahead of the recurrence, bit 6: never use the
 * gate-split form of the small-grid kernel (one gate per wave, for the smallest grids), bit 7: use its 8-wave form wherever the small-grid
 * kernel would run (bit-identical results either way). */
int vad_debug_set_conv_variant(int variant);
/* 0 = run the ConvLSTM layers strictly one after the other on the caller's stream; 1 (default) = small launch groups run
 * them as a wavefront: layer l step t on a library-owned helper stream as soon as layer l-1 step t is done (fork / join by
 * events on `stream`; the helper streams are created once per thread and device on the first such call).  Same results. */
int vad_debug_set_lstm_wavefront(int on);
/* Frames per dec4.0 -> scoring-tail sub-group inside vad_img_score (0 = whole launch group). */
int vad_debug_set_tail_group(int frames);
/* A/B: 0 = dec4.0 and the scoring tail of the image model as two launches (round-2 path), 1 = the fused kernel (default) */
int vad_debug_set_dec4_fused(int on);
/* rows of the dec3.3 map per work-group band of the fused kernel (0 = chosen from the batch size); results do not depend on it */
int vad_debug_set_dec4_band(int rows);
/* The CU count that every launch-planning decision sees: the choice between latency and throughput tilings, the small-grid
 * ConvLSTM and transposed-convolution forms, the band height of the fused tail and the grid of every persistent kernel
 * (CUs x resident work-groups).  0 (default) = the device's count; a value above it is refused (VAD_ERR_ARG).  With 1 a
 * handful of small frames runs the throughput tilings, and the persistent kernels walk many frames / items per work-group -
 * what the layer tests of tests/test_hip_persistent.py rely on.  Results never depend on it, except for the grouping of the
 * BatchNorm partial sums of the training forward.  Size bounds (vad_*_workspace_bytes, statistics rows) ignore it. */
int vad_debug_set_plan_cus(int cus);
/* This thread's latest persistent layer launch: out[0] grid work-groups, [1] work items (frame walkers: frames x tiles x column
 * blocks; item walkers: their item count), [2] independent walks (= the grid; 4 x the grid for the wave-persistent transposed
 * convolution / bf16 1x1 kernel), [3] kernel family (1 conv3x3 / ConvLSTM step, 2 fused first layer, 3 first layer, 4
 * convt2x2, 5 conv1x1 bf16, 6 fused dec4 tail, 7 Winograd), [4..7] the tiling MT, NT, WM, WN (conv families; dec4: band rows
 * and strips in [4], [5]), [8] the kernel mode (conv3x3: 0 plain, 1 pool, 2 ConvLSTM; convt2x2 / conv1x1: the VAD_PREC_* of
 * the instantiation; dec4: the input format; Winograd: 0 plain, 1 pool, 2 fused cell).  Grid 0: that launch was not persistent.
 * The record belongs to the entry points that have a persistent form - vad_conv3x3, vad_conv3x3_c3 (_fused, _bf16, _bf16op),
 * vad_convlstm_step, vad_convt2x2, vad_conv1x1_p, which clear it on entry, and vad_conv3x3_wino, vad_convlstm_step_wino,
 * vad_dec4_score, which always launch a persistent kernel; every other entry point (vad_conv1x1, the *_to3_score tails, the
 * BatchNorm / pooling passes, ...) leaves it as it was.
 * out[9..17]: the same nine values of the thread's latest PERSISTENT launch, whatever was launched behind it (the x halves of
 * a ConvLSTM sequence are followed by its steps).  Writes min(cap, 18) values and returns 18. */
int vad_debug_last_plan(int out[], int cap);
/* The statistics launches of the training forward, one layer at a time (the training steps call them internally): the
 * un-activated, un-pooled vad_conv3x3 / vad_convt2x2 / first-layer launch (cout 32; out16: 0 fp32 output, 1 bf16 output, 2 bf16
 * output and operands) that also writes its BatchNorm partial sums, stats[rows][2][cout] = per row the sums of (y - bias) and of
 * (y - bias)^2 over the outputs that row's work-group (convt2x2: wave) produced, and *rows = their count (0: this launch could
 * not provide them).  Room: vad_debug_stats_floats(kind, cout, n, h, w) floats, kind 0 conv3x3, 1 convt2x2, 2 first layer. */
size_t vad_debug_stats_floats(int kind, int cout, int n, int h, int w);
int vad_debug_conv3x3_stats(const float* in, long long in_fs, const float* w_packed, const float* bias, float* out, long long out_fs,
                            int n, int h, int w, int cin, int cout, int precision, float* stats, int* rows, void* stream);
int vad_debug_convt2x2_stats(const float* in, long long in_fs, const float* w_packed, const float* bias, float* out, long long out_fs,
                             int n, int h, int w, int cin, int cout, int precision, float* stats, int* rows, void* stream);
int vad_debug_conv3x3_c3_stats(const float* x_nchw, const float* w_packed, const float* bias, void* out, int out16, int n, int h, int w,
                               float* stats, int* rows, void* stream);

/* Row f-3 — raw-frame ingest.  The *_x forms take the original frames in either format:
 *   VAD_X_F32_NCHW (0): float32 [N,3,H,W] already normalised to [-1,1] (same as the plain entry points);
 *   VAD_X_U8_NHWC  (1): uint8 [N,H,W,3] as decoded from an image / video file.  ToTensor + Normalize(0.5, 0.5)
 *                       (reference utils/dataset.py:65-70, utils/video_dataset.py:62-66) is applied inside the first
 *                       convolution's staging load and inside the scoring tail, bit-identically to the fp32 path, so
 *                       the normalised fp32 frames (4x the bytes) never exist in memory.
 * `precision` is the arithmetic mode the blob was packed for (VAD_PREC_*).  All other arguments and outputs are those of
 * vad_img_score / vad_vid_score / vad_vid_score_windows (which are the float-input, VAD_PREC_FP32 short forms). */
#define VAD_X_F32_NCHW 0
#define VAD_X_U8_NHWC 1
int vad_img_score_x(const void* x, int x_format, int precision, long long b, int h, int w, int latent, const float* packed_dev,
                    void* workspace, size_t workspace_bytes, int chunk, float* scores, float* errmap, float* recon_nchw,
                    float* latent_nchw, void* stream);
int vad_vid_score_x(const void* x, int x_format, int precision, long long b, int t, int h, int w, int latent, int hid, int layers,
                    const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk_clips, float* seq_scores,
                    float* frame_scores, float* errmap, float* recon, void* stream);
int vad_vid_score_windows_x(const void* frames, int x_format, int precision, long long nframes, int t, int stride, int h, int w,
                            int latent, int hid, int layers, const float* packed_dev, void* workspace,
                            size_t workspace_bytes, int chunk_windows, float* seq_scores, float* frame_scores,
                            float* errmap, float* recon, void* stream);

/* Dense sliding-window scoring of ONE video: window k = frames [k*stride, k*stride + T), 0 < stride <= T,
 * vad_vid_num_windows(F, T, stride) = (F - T) / stride + 1 windows.  Same results as scoring every window as its own
 * clip with vad_vid_score (what the reference does: evaluate_video.py:322-352 builds VideoFileDataset(sequence_length,
 * stride=1) and runs 3 forwards per window), but every frame is encoded once instead of once per window containing it.
 * frames [F,3,H,W].  Outputs (any may be NULL): seq [NW]; frame [NW,T]; errmap [NW,T,H,W]; recon [NW,T,3,H,W]. */
long long vad_vid_num_windows(long long frames, int t, int stride);
size_t vad_vid_windows_workspace_bytes(int chunk_windows, int t, int stride, int h, int w, int latent, int hid, int layers);
int vad_vid_score_windows(const float* frames, long long nframes, int t, int stride, int h, int w, int latent, int hid,
                          int layers, const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk_windows,
                          float* seq_scores, float* frame_scores, float* errmap, float* recon, void* stream);

/* Models with in_channels > 3 (round 4).  ConvAutoencoder(in_channels=...) / VideoAutoencoder(in_channels=...) take any width
 * (models/autoencoder.py:161, models/video_autoencoder.py:290-296; every reference call site passes 3: evaluate.py:35,
 * evaluate_video.py:99-104).  The `_c` forms below take in_ch in [3, VAD_MAX_IN_CHANNELS]; with in_ch == 3 they ARE the forms
 * above.  A wider model runs its first and last layer on the generic kernels over planes zero-padded to 32 channels
 * (csrc/wide_io.hip: one NCHW -> padded-NHWC copy on the way in, Tanh + squared error on the way out); blobs come from
 * vad_img_pack(..., in_ch, ...) / vad_vid_pack_c, inputs are float NCHW [.., in_ch, H, W] (uint8 frames are 3-channel
 * images), recon comes back with in_ch planes, scores and error maps average over in_ch planes.  1- and 2-channel models: pack
 * and score them as 3-channel models with zero weights on the extra planes (what the Python layer does). */
#define VAD_MAX_IN_CHANNELS 32
size_t vad_img_workspace_bytes_c(int chunk, int h, int w, int latent, int in_ch);
int vad_img_score_c(const void* x, int x_format, int precision, int in_ch, long long b, int h, int w, int latent,
                    const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk, float* scores, float* errmap,
                    float* recon_nchw, float* latent_nchw, void* stream);
size_t vad_vid_packed_floats_c(int in_ch, int latent, int hid, int layers);
int vad_vid_pack_c(const float* const* params, int nparams, int in_ch, int latent, int hid, int layers, int precision,
                   float* packed_host);
size_t vad_vid_workspace_bytes_c(int chunk_clips, int t, int h, int w, int latent, int hid, int layers, int in_ch);
int vad_vid_score_c(const void* x, int x_format, int precision, int in_ch, long long b, int t, int h, int w, int latent, int hid,
                    int layers, const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk_clips,
                    float* seq_scores, float* frame_scores, float* errmap, float* recon, void* stream);
size_t vad_vid_windows_workspace_bytes_c(int chunk_windows, int t, int stride, int h, int w, int latent, int hid, int layers,
                                         int in_ch);
int vad_vid_score_windows_c(const void* frames, int x_format, int precision, int in_ch, long long nframes, int t, int stride,
                            int h, int w, int latent, int hid, int layers, const float* packed_dev, void* workspace,
                            size_t workspace_bytes, int chunk_windows, float* seq_scores, float* frame_scores, float* errmap,
                            float* recon, void* stream);

/* ------------------------------------------------------------------ recurrent state carried across calls
 * ConvLSTM.forward(x, hidden_state) takes an initial state and returns the final one (models/video_autoencoder.py:127-166);
 * a live stream is scored a frame (or a few) per call, for O(1) work per frame, by carrying that state.
 *
 * State blob (caller-owned device memory, 16-B aligned, fp32, the kernels' own layout):
 *     for l in 0..layers-1:  h_l [B][GH][GW][hid_p]  then  c_l [B][GH][GW][hid_p]        (NHWC, dense)
 * GH x GW is the ConvLSTM's grid (H/16 x W/16 of the video model), hid_p the hidden width zero-padded to a multiple of 64
 * (the padded channels hold exact zeros and stay zero).  vad_vid_state_floats / vad_convlstm_state_floats give its size, 0 for
 * unsupported shapes.  A blob is valid ONLY for the (B, H, W, hid, layers) it was sized for: row i belongs to stream i of a
 * B-stream call, and a launch group [c0, c0+nc) of a chunked call reads and writes rows c0..c0+nc-1 of every plane.  Zero-filled
 * memory is the zero state.  The library keeps no state of its own: two streams or threads share nothing.
 *
 * In-place rule: state_in == state_out is allowed.  Step 0 of every layer reads state_in; state_out is written once per
 * launch group after all of that group's steps have run, so an aliased blob is updated only after its last reader.
 * state_in == NULL is the zero state and takes exactly the launches of the stateless call; state_out == NULL discards. */
size_t vad_vid_state_floats(int b, int h, int w, int hid, int layers);
size_t vad_convlstm_state_floats(int b, int gh, int gw, int hid_p, int layers);
/* vad_vid_score_c plus the state: x [B,T,in_ch,H,W] (or uint8 [B,T,H,W,3]) continues B streams by T frames each.  Every
 * arithmetic mode, ingest format, in_ch, proj / layer count and chunking of vad_vid_score_c; T >= 1; the workspace is sized by
 * vad_vid_workspace_bytes_c for THIS call's T.  Scoring a clip in one call or in pieces with the state carried gives the same
 * bits.  vad_vid_score_c(...) is vad_vid_score_s(..., NULL, NULL, stream). */
int vad_vid_score_s(const void* x, int x_format, int precision, int in_ch, long long b, int t, int h, int w, int latent, int hid,
                    int layers, const float* packed_dev, void* workspace, size_t workspace_bytes, int chunk_clips,
                    float* seq_scores, float* frame_scores, float* errmap, float* recon,
                    const float* state_in, float* state_out, void* stream);
/* Blob <-> the reference's tensors for one layer: h, c NCHW [B, hid, GH, GW] with the REAL width hid <= hid_p.  Import writes
 * exact zeros into the padded channels, export drops them (csrc/state_io.hip: LDS-staged, both sides coalesced). */
int vad_state_import(const float* h_nchw, const float* c_nchw, float* state, int layer, int b, int gh, int gw, int hid, int hid_p,
                     int layers, void* stream);
int vad_state_export(const float* state, float* h_nchw, float* c_nchw, int layer, int b, int gh, int gw, int hid, int hid_p,
                     int layers, void* stream);
/* The same converters on plain frame batches: NCHW [n, c, h, w] <-> NHWC [n, h, w, cpad], cpad >= c a multiple of 4. */
int vad_nchw_to_nhwc_padded(const float* in, float* out, long long n, int h, int w, int c, int cpad, void* stream);
int vad_nhwc_padded_to_nchw(const float* in, float* out, long long n, int h, int w, int c, int cpad, void* stream);

/* Layer-level roll-out: ConvLSTM(input_dim, hidden_dims).forward(x, hidden_state) (models/video_autoencoder.py:94-179) - the
 * ConvLSTM block of vad_vid_score_s as an entry point of its own (one launch sequence serves both).  The reference takes one
 * hidden width per layer; every layer runs at ONE padded width hid_p (that of the widest, vad_convlstm_padded_dims), cin_p is
 * the padded input width.  vad_convlstm_pack: params = (weight (4*hid_l, in_l + hid_l, 3, 3), bias) per cell, host pointers.
 * x [B][T][GH][GW][cin_p] NHWC (padded channels zero).  hseq_out: the h sequence [B][T][GH][GW][hid_p] of the last layer, or
 * with all_layers != 0 of every layer ([layers][B][T]...).  state_in / state_out: blobs of vad_convlstm_state_floats(b, gh, gw,
 * hid_p, layers), NULL = zero state / discard, may alias.  precision: VAD_PREC_FP32; VAD_PREC_SPLIT / _WINO need cin_p == hid_p. */
int vad_convlstm_padded_dims(int cin, const int* hids, int layers, int* cin_p, int* hid_p);
size_t vad_convlstm_packed_floats(int cin_p, int hid_p, int layers);
int vad_convlstm_pack(const float* const* params, int nparams, int cin, const int* hids, int layers, int precision,
                      float* packed_host);
size_t vad_convlstm_seq_workspace_bytes(int b, int t, int gh, int gw, int cin_p, int hid_p, int layers, int all_layers);
int vad_convlstm_seq(const float* x, int precision, long long b, int t, int gh, int gw, int cin_p, int hid_p, int layers,
                     const float* packed_dev, void* workspace, size_t workspace_bytes, float* hseq_out, int all_layers,
                     const float* state_in, float* state_out, void* stream);

/* ------------------------------------------------------------------ Resize of uint8 frames (csrc/resize_u8.hip)
 * `transforms.Resize((S, S))` on a PIL image - the first step of every input pipeline of the reference (utils/dataset.py:65-70,
 * utils/video_dataset.py:62-66, 191-195, 356-360, main.py:209-218) - is PIL's `Image.resize((S, S), BILINEAR)`: an antialiased,
 * separable, integer fixed-point resample on uint8.  vad_resize_u8 reproduces it BIT FOR BIT on the device: src uint8
 * [n, in_h, in_w, 3] (contiguous, as decoded) -> dst uint8 [n, out_h, out_w, 3], always RGB, i.e. the VAD_X_U8_NHWC form the
 * scoring entry points take.  channel_order: 0 = src is RGB, 1 = src is BGR (what cv2.VideoCapture delivers; the reference
 * converts with cv2.cvtColor first, utils/video_dataset.py:284, 389) - the swap happens on the load and is exact.
 *
 * Supported geometries: input sides 1..16384, output sides 1..4096, and on each axis in <= 64 * out; everything else is
 * refused (vad_resize_plan_bytes returns 0).  out_h / out_w need not be multiples of 16 here (that is the models' rule).
 *
 * Plan: the coefficient tables of one geometry, computed once on the host in double (vad_resize_plan needs no GPU) and
 * uploaded by the caller, who owns it like a packed weight blob (the library keeps no state); int32 words, 16-B aligned on the
 * device, vad_resize_plan_bytes bytes (a few KB to ~200 KB).  It starts with a tagged header carrying the four sizes.  The
 * sizes are ALSO arguments of vad_resize_u8: the host validates them, and every kernel compares them with the header ON THE
 * DEVICE - with a plan made for another geometry (or not a plan at all) dst is filled with zeros, never with pixels, and no
 * offset of that blob is followed.
 *
 * Workspace: the horizontal pass's uint8 result [n, rows the vertical pass reads, out_w, 3]; vad_resize_workspace_bytes (0 when
 * at most one axis changes: NULL is then accepted).  A pass whose lengths are equal is skipped; with both equal dst is a copy. */
size_t vad_resize_plan_bytes(int in_h, int in_w, int out_h, int out_w);                       /* 0 = unsupported geometry */
int vad_resize_plan(int in_h, int in_w, int out_h, int out_w, void* plan_host);               /* host only */
size_t vad_resize_workspace_bytes(long long n, int in_h, int in_w, int out_h, int out_w);
int vad_resize_u8(const void* src, long long n, int in_h, int in_w, int channel_order, const void* plan_dev, void* dst, int out_h,
                  int out_w, void* workspace, size_t workspace_bytes, void* stream);

/* The same Resize for the other pixel layouts a decoder delivers (the reference opens every file with
 * `Image.open(path).convert('RGB')`, utils/dataset.py:141, utils/video_dataset.py:141, 295, main.py:218, and the MVTec masks with
 * `convert('L')` + `mask_transform`, utils/dataset.py:74-77, 147-148).  Exact by construction: PIL's L -> RGB replicates the
 * channel, RGBA -> RGB drops alpha, and the resample treats channels independently.
 *   pixel_format   src (uint8, contiguous)                          dst (uint8)
 *   VAD_PIX_RGB    [n, in_h, in_w, 3]                               [n, out_h, out_w, 3]   = vad_resize_u8, channel_order 0
 *   VAD_PIX_BGR    [n, in_h, in_w, 3]                               [n, out_h, out_w, 3]   = vad_resize_u8, channel_order 1
 *   VAD_PIX_L      [n, in_h, in_w]       one byte per pixel         [n, out_h, out_w, out_channels]: out_channels 3 = the resized
 *                                                                   plane in all three channels (`convert('RGB')`), 1 = the plane (masks)
 *   VAD_PIX_RGBA   [n, in_h, in_w, 4]    fourth byte ignored        [n, out_h, out_w, 3]
 *   VAD_PIX_BGRA   [n, in_h, in_w, 4]    fourth byte ignored        [n, out_h, out_w, 3], B and R exchanged as VAD_PIX_BGR does
 * out_channels is 3, or 1 with VAD_PIX_L; anything else, and an unknown format, is refused before any launch.  The plan blob is
 * the one vad_resize_plan makes (the coefficients depend on the axis lengths only), with the same host checks and the same
 * on-device header check: a plan of another geometry gives zeros.  Workspace: the horizontal pass's result, ONE byte per pixel
 * for VAD_PIX_L (the value is replicated on the last store) and three otherwise; vad_resize_workspace_bytes_f (0 for arguments
 * the launcher refuses and when at most one axis changes).  With both passes skipped dst is the replicated / alpha-stripped /
 * swapped copy. */
#define VAD_PIX_RGB 0
#define VAD_PIX_BGR 1
#define VAD_PIX_L 2
#define VAD_PIX_RGBA 3
#define VAD_PIX_BGRA 4
size_t vad_resize_workspace_bytes_f(long long n, int in_h, int in_w, int out_h, int out_w, int pixel_format, int out_channels);
int vad_resize_u8_f(const void* src, long long n, int in_h, int in_w, int pixel_format, const void* plan_dev, void* dst, int out_h,
                    int out_w, int out_channels, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ Frame bank -> batch (csrc/frame_gather.hip)
 * Decoded, resized uint8 frames stay resident in HBM (`bank`, [bank_frames, h, w, 3] contiguous; it may point into the middle
 * of a larger allocation, at any byte address) and every batch is ONE gather: output frame i = bank frame index[i], so the
 * overlapping sequences of the reference's datasets (utils/video_dataset.py:113-131, 240-247) are index entries, not copies.
 *   VAD_X_F32_NCHW  out float32 [n, 3, h, w], each value ToTensor + Normalize(0.5, 0.5) of its byte, the bits of
 *                   (u8/255 - 0.5)/0.5 evaluated step by step in fp32 - what the float entry points and the trainers take
 *   VAD_X_U8_NHWC   out uint8 [n, h, w, 3], a plain copy - what the uint8 ingest of the scoring entry points takes
 * index: device int64 [n].  An entry outside [0, bank_frames) is the caller's error: that output frame is neither read for nor
 * written (it keeps what it held), nothing is read out of bounds, and the call still returns VAD_OK - the host cannot see the
 * device's indices without a synchronisation, so validate them before upload.  Any h, w >= 1 (h * w <= 2^27); 16-byte accesses
 * are used where the addresses allow, a plain path otherwise.  n == 0 returns VAD_OK and launches nothing.  One launch on
 * `stream`, no allocation, no host synchronisation: capturable in a graph. */
int vad_gather_frames_u8(const unsigned char* bank, long long bank_frames, const long long* index, long long n, int h, int w,
                         int out_format, void* out, void* stream);

/* ------------------------------------------------------------------ Score histogram (csrc/score_hist.hip)
 * The joint distribution of (score, label) as integer counters: everything a ranking metric needs - pixel-level AUROC of an
 * error map / SSIM map against the ground-truth mask the reference only plots (evaluate.py:142-171), frame-level AUROC
 * (evaluate_video.py:171-176) - accumulated batch by batch on the device; only the counters are ever read by the host.
 *
 * Quantiser, one parameter m = mantissa_bits in [VAD_HIST_MIN_M, VAD_HIST_MAX_M]: a finite v >= 0 (-0.0 counts as 0) falls into
 * bin key(v) = float_bits(v) >> (23 - m), of (255 << m) bins; a <= b implies key(a) <= key(b).  A negative value, a NaN or an
 * infinity is not binned: it increments rejected[class].
 *
 * State blob (caller-owned device memory, 16-byte aligned, vad_hist_state_bytes(m) bytes; 0 for an m out of range):
 *     uint32 header[4] = {magic "VADH", abi << 16 | m, m, 0};  uint64 counts[2][nbins];  uint64 rejected[2]     (class 0, 1)
 * vad_hist_reset writes the header and zeroes the counters.  The host checks every argument it can see and returns VAD_ERR_ARG;
 * the header lives in device memory, so - as for the model and resize blobs - every kernel compares it with the call's m ON THE
 * DEVICE: with a state made for another m (or not a state) the call changes nothing, and no offset of that blob is followed.
 * Integer atomics only: the counters are exact, and identical for any batching, launch order or sharding.  All calls are
 * asynchronous on `stream`, allocate nothing and can be captured into a graph.
 *
 * vad_hist_accumulate: values = n_groups * group_elems contiguous fp32 (4-byte aligned; any count), labels in label_format:
 *   VAD_LBL_U8_ELEM   one byte per element, positive iff >= 128
 *   VAD_LBL_F32_ELEM  one float per element, positive iff > 0.5   (what ToTensor makes of a mask: b / 255 > 0.5 iff b >= 128)
 *   VAD_LBL_U8_GROUP  one byte per group, positive iff non-zero, applied to the group's group_elems elements (a frame's label for
 *                     its pixels; group_elems = 1: a vector of frame scores)
 * vad_hist_merge: dst += src, counts and rejected (two streams, or the states of several ranks after a gather). */
#define VAD_HIST_MIN_M 4
#define VAD_HIST_MAX_M 15
#define VAD_LBL_U8_ELEM 0
#define VAD_LBL_F32_ELEM 1
#define VAD_LBL_U8_GROUP 2
size_t vad_hist_state_bytes(int m);
int vad_hist_reset(void* state, int m, void* stream);
int vad_hist_accumulate(const float* values, long long n_groups, long long group_elems, const void* labels, int label_format,
                        void* state, int m, void* stream);
int vad_hist_merge(void* dst, const void* src, int m, void* stream);

/* ------------------------------------------------------------------ Per-region overlap (csrc/region_overlap.hip)
 * The localisation metric of MVTec-style data: PRO(t) = the mean, over all connected anomalous regions r of the ground-truth
 * masks, of |{p in r : v_p >= t}| / |r|, against FPR(t) over all normal pixels; AUPRO integrates the curve up to a false-positive
 * rate (0.3) on the host, from counters.  The device labels the masks and accumulates the counters; maps, masks, labels and
 * region sizes never leave it.
 *
 * vad_label_regions: masks = n images of h x w (any h, w >= 1 with h * w < 2^31 - 1; n * h * w <= 2^38), a pixel anomalous under
 * VAD_LBL_U8_ELEM (>= 128) or VAD_LBL_F32_ELEM (> 0.5); connectivity 8 (the 3 x 3 structure of the MVTec evaluation) or 4.  Every
 * image is labelled on its own.  labels int32 [n, h, w]: 0 = normal, otherwise 1 + (the smallest y * w + x of the pixel's region) -
 * canonical, so two labellings compare element by element.  sizes_or_null uint32 [n, h, w]: the region's pixel count at the
 * region's root pixel (the one whose label is its own index + 1), 0 elsewhere.  ws: caller-provided, 16-byte aligned,
 * vad_pro_workspace_bytes(n, h, w) bytes (0 for dimensions out of range); its first uint32 is a flag word the call clears and the
 * kernels set: every walk of the union-find is bounded by a step count known at launch (2 * h * w), and a walk that exhausts it
 * sets bit 0 and leaves - a defect gives a wrong labelling and a set flag, never a hang.  n == 0 clears the flag word only.
 *
 * State blob (caller-owned, 16-byte aligned, vad_pro_state_bytes(m) bytes; 0 for an m out of range; m and the quantiser as above):
 *     uint32 header[4] = {magic "VADP", abi << 16 | m, m, 0};  uint64 wpos[nbins], pos[nbins], neg[nbins];
 *     uint64 regions, max_region, rejected[2], flags
 * vad_pro_accumulate labels the masks into ws and adds the batch: a normal pixel 1 to neg[key(v)]; an anomalous pixel of region r
 * 1 to pos[key(v)] and W(r) = (2^VAD_PRO_WEIGHT_BITS + |r| / 2) / |r| (integer division) to wpos[key(v)]; a negative, NaN or
 * infinite value 1 to rejected[class] (it still counts towards |r|); the number of regions to `regions`; the largest |r| into
 * max_region; the workspace's flag word into flags.  One region adds at most 2^44 + |r| / 2 to a bin, so a bin cannot wrap below
 * 2^19 regions: the reader of the counters checks `regions` (accumulating cannot).  pos / neg are what vad_hist_accumulate counts.
 * Integer atomics only: exact, and identical for any batching, launch order or sharding.  The header is compared with m ON THE
 * DEVICE: with a foreign blob the call changes nothing and follows no offset of it.  vad_pro_merge: dst += src; the maximum for
 * max_region, the union for flags.  All calls are asynchronous on `stream`, allocate nothing and can be captured into a graph. */
#define VAD_PRO_WEIGHT_BITS 44
size_t vad_pro_state_bytes(int m);
int vad_pro_reset(void* state, int m, void* stream);
int vad_pro_merge(void* dst, const void* src, int m, void* stream);
size_t vad_pro_workspace_bytes(long long n, int h, int w);
int vad_label_regions(const void* masks, int label_format, long long n, int h, int w, int connectivity, int32_t* labels,
                      uint32_t* sizes_or_null, void* ws, size_t ws_bytes, void* stream);
int vad_pro_accumulate(const float* values, const void* masks, int label_format, long long n, int h, int w, int connectivity,
                       void* state, int m, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ Smoothed anomaly maps (csrc/map_smooth.hip)
 * The two steps an MVTec-style evaluation takes between the error map and the ranking metrics: the map is smoothed with a Gaussian
 * (scipy.ndimage.gaussian_filter, conventionally sigma = 4) and the image is scored by the maximum of the smoothed map.
 *
 * vad_smooth_maps: maps = n frames of h x w fp32, contiguous (any h, w >= 1 with h * w <= VAD_MAX_FRAME_PIXELS; 4-byte aligned).
 * taps_dev: device fp32 [2 * radius + 1], made on the host (scipy's: w[k] = exp(-0.5 / sigma^2 * (k - radius)^2) in float64,
 * divided by their float64 sum, rounded once to fp32; every tap must be > 0).  Borders: scipy's mode="reflect" (index -k -> k - 1,
 * index n - 1 + k -> n - k), one reflection, so radius <= min(h, w).  First along h, then along w; each pass is
 * acc = fl(w[0] x[0]), acc = fl(acc + fl(w[k] x[k])) for k = 1 .. 2 radius ascending, every product and sum rounded to fp32 on its
 * own (no fused multiply-add), the intermediate fp32: numpy float32 restates it bit for bit.  A NaN makes exactly the pixels whose
 * reflected window holds it NaN; +Inf spreads as +Inf.
 * out (may be NULL): n x h x w smoothed maps; it must not overlap maps.  frame_max (may be NULL; not both): [n], the maximum of
 * each smoothed frame with torch.amax semantics (NaN if any pixel of the frame is) - compare-only, the same for every batching,
 * launch order and tiling.  ws: vad_smooth_workspace_bytes(n, h, w, radius) bytes (0 for arguments out of range), needed only with
 * frame_max (VAD_ERR_WS when smaller).  VAD_ERR_ARG for radius outside 1 .. VAD_SMOOTH_MAX_RADIUS or above min(h, w), n < 0, both
 * outputs NULL, out overlapping maps, a misaligned pointer.  n == 0 returns VAD_OK and launches nothing.  One launch (two with
 * frame_max) on `stream`, no allocation, no host synchronisation: capturable in a graph.
 * vad_smooth_tile reports the output tile of one work-group (rows, columns) - what a test needs to build a frame of several tiles. */
#define VAD_SMOOTH_MAX_RADIUS 32
size_t vad_smooth_workspace_bytes(long long n, int h, int w, int radius);
int vad_smooth_maps(const float* maps, long long n, int h, int w, const float* taps_dev, int radius, float* out, float* frame_max,
                    void* ws, size_t ws_bytes, void* stream);
int vad_smooth_tile(int* tile_h, int* tile_w);

/* ------------------------------------------------------------------ Order statistics and top-k means of anomaly maps (csrc/map_topk.hip)
 * The robust frame scores between the mean of a map (a small defect barely moves it) and its maximum (one pixel decides): the k-th
 * largest pixel - a quantile - and the mean of the k largest pixels, for up to VAD_TOPK_MAX_RANKS ranks in one call.
 *
 * vad_map_topk: maps = n frames of h x w fp32, contiguous (any h, w >= 1 with P = h * w <= VAD_MAX_FRAME_PIXELS; 4-byte aligned).
 * ranks: nk values in HOST memory (nk in 1 .. VAD_TOPK_MAX_RANKS), each in 1 .. P; rank k means the k-th largest.  Any order and
 * duplicates are allowed: every column is independent of the others.  The ranks are read at call time and travel as kernel
 * arguments, so a captured call replays with the ranks it was captured with.
 * Pixels are ordered by the monotone key of their bits, key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), compared unsigned:
 * -inf < ... < -0.0 < +0.0 < ... < +inf; a tie between -0.0 and +0.0 is decided.
 * kth (may be NULL) [n, nk]: kth[i, j] is the pixel of frame i whose key is the ranks[j]-th largest, its bits unchanged.
 * topk_mean (may be NULL; not both) [n, nk]: (float)((S + (double)(k - c) * (double)v) / (double)k) with k = ranks[j], v = kth[i, j],
 * c = the number of pixels of the frame with key > key(v) and S = the float64 sum of those c pixels - every term is exact in double,
 * the order of the additions is the kernel's and is fixed, so S is within c * 2^-53 * sum|x| of the exact sum and the mean within
 * half a float32 spacing more.  IEEE double arithmetic decides the infinities: a +inf among the k largest gives +inf, both signs NaN.
 * A frame with any NaN pixel gets the canonical quiet NaN (0x7FC00000) in every output, torch.amax's rule and frame_max's above; no
 * other frame changes a bit.  A frame's outputs are the same words for any n, any position in the batch, any contents of the other
 * frames, eager or replayed: integer atomics on counters only, sums folded in a fixed order, no work-group reads another's results.
 * ws: caller-provided, 16-byte aligned, vad_topk_workspace_bytes(n, h, w, nk) bytes (0 for arguments out of range; no device is
 * needed).  It begins with 16 bytes per frame and rank, the record the outputs were formed from - uint32 bits of v, uint32 c, double
 * S (a NaN frame: 0x7FC00000, 0, NaN); frames above the split boundary add 80 bytes of state and nk tables of 8 KiB per frame and
 * 8 bytes per slice, frame and rank.  VAD_ERR_ARG for both outputs NULL, nk out of range, a rank of 0 or above P, n < 0 (or above
 * 2^56), h or w out of range, a NULL or misaligned pointer, an output overlapping maps; VAD_ERR_WS for a short workspace.  n == 0
 * returns VAD_OK and launches nothing.  Three reads of the maps.  Frames of at most `split_above` pixels: one launch, one work-group
 * per frame.  Larger frames - which one CU would read for milliseconds - are split into slices of `slice_pixels` pixels, one
 * work-group each: a memset and six launches (per digit a histogram launch that adds integer counters into the frame's tables and
 * a pick launch; the slices' float64 sums are added in slice order).  All on `stream`, no allocation, no host synchronisation:
 * capturable in a graph.
 * vad_topk_plan reports the boundary between the two paths and the slice - what a test needs to put a frame on each side. */
#define VAD_TOPK_MAX_RANKS 8
size_t vad_topk_workspace_bytes(long long n, int h, int w, int nk);
int vad_topk_plan(int* split_above, int* slice_pixels);
int vad_map_topk(const float* maps, long long n, int h, int w, const unsigned* ranks, int nk, float* kth, float* topk_mean,
                 void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ Grey morphology of anomaly maps (csrc/map_morph.hip)
 * The clean-up between the map and its threshold: an opening removes speckle that no Gaussian removes without blurring real
 * defects, a closing fills pinholes and joins the fragments of one defect.  Flat rectangular structuring element.
 *
 * vad_morph_maps: maps = n frames of h x w fp32, contiguous (any h, w >= 1 with h * w <= VAD_MAX_FRAME_PIXELS; 4-byte aligned).
 * The structuring element is size_h x size_w, each side in 1 .. VAD_MORPH_MAX_SIZE, even sizes included; a side may exceed h or w.
 * Semantics: scipy.ndimage.grey_erosion / grey_dilation / grey_opening / grey_closing with size=(size_h, size_w), mode="reflect" -
 * for a flat element, windows clamped to the image with scipy's even-size convention; per axis of length L and size s
 *   VAD_MORPH_ERODE   out[i] = min x[max(0, i - s/2)       .. min(L - 1, i + (s - 1)/2)]
 *   VAD_MORPH_DILATE  out[i] = max x[max(0, i - (s - 1)/2) .. min(L - 1, i + s/2)]
 *   VAD_MORPH_OPEN    dilate(erode(x)),   VAD_MORPH_CLOSE   erode(dilate(x));  the second step clamps its windows to the image on
 *                     the intermediate image, which has no values outside the frame.
 * Nothing is rounded; min and max are the IEEE-754-2019 minimum / maximum: a NaN makes exactly the pixels whose window holds it NaN
 * (open / close: the windows of both steps), -0 orders below +0, +-Inf are ordinary values.  Size 1 x 1 is a copy.  Because the
 * operations only compare, they commute with a threshold: op(x) >= t is the binary op of x >= t.
 * out: n x h x w; it must not overlap maps.  VAD_ERR_ARG for an unknown op, a size outside 1 .. VAD_MORPH_MAX_SIZE, n < 0, h or w
 * out of range, a NULL or misaligned pointer, out overlapping maps.  n == 0 returns VAD_OK and launches nothing.  One launch per
 * call (open and close included) on `stream`, one read and one write of the maps, no workspace, no allocation, no host
 * synchronisation: capturable in a graph.
 * vad_morph_tile reports the output tile of one work-group (rows, columns) for a size and op - what a test needs to build a frame of
 * several tiles; VAD_ERR_ARG for an unknown op or a size out of range. */
#define VAD_MORPH_MAX_SIZE 31
enum { VAD_MORPH_ERODE = 0, VAD_MORPH_DILATE = 1, VAD_MORPH_OPEN = 2, VAD_MORPH_CLOSE = 3 };
int vad_morph_maps(const float* maps, long long n, int h, int w, int op, int size_h, int size_w, float* out, void* stream);
int vad_morph_tile(int size_h, int size_w, int op, int* tile_h, int* tile_w);

/* ------------------------------------------------------------------ Rank filters of anomaly maps (csrc/map_rankfilt.hip)
 * The sliding-window median and its generalisation, the r-th smallest value of a rectangular window: the denoiser of impulsive
 * noise (single hot pixels) that keeps step edges where they are and leaves the level of flat areas alone.  Erosion and dilation
 * above are the two end ranks of this family.
 *
 * vad_rankfilt_maps: maps = n frames of h x w fp32, contiguous (any h, w >= 1 with h * w <= VAD_MAX_FRAME_PIXELS; 4-byte aligned).
 * The window is size_h x size_w (N = size_h * size_w values), each side in 1 .. VAD_RANKFILT_MAX_SIZE, even sizes included; a side
 * may exceed h or w.  rank is 0-based and ascending, 0 .. N - 1.
 * Semantics: scipy.ndimage.rank_filter(x, rank, size=(size_h, size_w), mode="reflect") -
 *   out[y][x] = the rank-th smallest of { x[R(y - size_h/2 + i, h)][R(x - size_w/2 + j, w)] : 0 <= i < size_h, 0 <= j < size_w }
 *   R(i, L): m = i mod 2L (non-negative);  m < L ? m : 2L - 1 - m          (d c b a | a b c d | d c b a, periodic)
 * with integer division: even sizes lean towards index 0, as VAD_MORPH_ERODE does.  A reflected pixel counts as often as it appears
 * in the window (a rank, unlike a minimum or maximum, cannot clamp its window); a window larger than the frame reflects several
 * times.  median_filter is rank = N / 2 (the upper median of an even N); percentile_filter(p) is p += 100 if p < 0, then rank =
 * N - 1 if p == 100, else (int)((double)N * p / 100.0).
 * Relations to vad_morph_maps: rank 0 equals VAD_MORPH_ERODE at every size.  Rank N - 1 equals VAD_MORPH_DILATE at ODD sizes only:
 * scipy's dilation mirrors the origin of an even element (it reaches (s - 1) / 2 towards index 0, this window s / 2).
 * Nothing is computed, only selected, so the result is specified to the bit: the order is that of the monotone integer key of
 * vad_map_topk (-0 below +0; denormals and +-Inf are ordinary values), the result is one of the window's values with its bits
 * unchanged, and a window that holds a NaN gives NaN at every rank, as vad_morph_maps does (scipy's result there is an accident of
 * its selection algorithm and is not followed).  Size 1 x 1 is a copy.
 * out: n x h x w; it must not overlap maps.  VAD_ERR_ARG for a size outside 1 .. VAD_RANKFILT_MAX_SIZE, a rank outside 0 .. N - 1,
 * n < 0, h or w out of range, a NULL or misaligned pointer, out overlapping maps.  n == 0 returns VAD_OK and launches nothing.
 * One launch per call on `stream` (n above 65535: one per 65535 frames, as vad_morph_maps), one read and one write of the maps, no
 * workspace, no allocation, no host synchronisation: capturable in a graph.  A frame's bits do not depend on its batch.
 * vad_rankfilt_tile reports the output tile of one work-group (rows, columns) for a size - what a test needs to build a frame of
 * several tiles; VAD_ERR_ARG for a size out of range. */
#define VAD_RANKFILT_MAX_SIZE 15
int vad_rankfilt_maps(const float* maps, long long n, int h, int w, int size_h, int size_w, int rank, float* out, void* stream);
int vad_rankfilt_tile(int size_h, int size_w, int* tile_h, int* tile_w);

/* ------------------------------------------------------------------ Temporal filters of anomaly maps (csrc/map_temporal.hip)
 * The step a video line takes between the map and its threshold: every pixel filtered over the last k frames of its stream.  The
 * minimum is a temporal erosion ("high in each of the last k frames": removes noise that differs from frame to frame, without any
 * spatial blur), the maximum a temporal dilation (holds a detection across a dropped frame), the mean and the exponential average
 * lower the noise floor of a fixed camera.  Per pixel, causal, windowed over the frames that exist.
 *
 * Frames of one stream are x[0], x[1], ...; frame 0 is the first after vad_tfilt_init, or the first of a clip.
 *   VAD_TFILT_MIN / MAX  y[t] = minimum / maximum of x[max(0, t - k + 1) .. t], k in 1 .. VAD_TFILT_MAX_K: scipy.ndimage.
 *                        minimum_filter1d / maximum_filter1d(x, size=k, axis=0, mode="nearest", origin=(k - 1) // 2).  The IEEE-754-2019
 *                        minimum / maximum: a NaN makes exactly the k outputs whose window holds it NaN, -0 orders below +0, +-Inf are
 *                        ordinary values.  Nothing is rounded; k = 1 is a copy.  They only compare, so they commute with a threshold.
 *   VAD_TFILT_MEAN       y[t] = (float)(S / (double)c), c = min(t + 1, k), S the float64 sum of the window's values added oldest to
 *                        newest, formed anew for every output; one rounding to float32 at the end.  Within 2^-24 |m| + 2^-150 +
 *                        (c + 1) 2^-53 sum|x| / c of the exact mean m.  NaN / Inf follow the arithmetic.
 *   VAD_TFILT_EMA        y[0] = x[0], y[t] = y[t-1] + a * (x[t] - y[t-1]) with a = alpha (float32, 0 < a < 1), every operation rounded
 *                        to float32 on its own, no fused multiply-add: a finite constant stream stays constant to the bit (-0 becomes +0, an
 *                        infinity NaN: x - y is then +0 or NaN).  A NaN stays in
 *                        the state until the stream is initialised again - never a finite wrong value.  k is not used.
 * vad_tfilt_maps: maps fp32 [b, t, h, w], contiguous, 4-byte aligned (b in 0 .. 2^20, t >= 0, any h, w >= 1 with h * w <=
 * VAD_MAX_FRAME_PIXELS) are the next t frames of b streams; out [b, t, h, w] must not overlap maps.  state_or_null == NULL is the
 * clip mode: every one of the b clips is a fresh stream, nothing is carried; it gives the bits a freshly initialised state gives.
 * The result of a stream does not depend on how its frames are split over calls.
 * State (caller-owned device memory, 16-byte aligned, vad_tfilt_state_bytes(b, h, w, op, k) bytes; 0 for arguments out of range, no
 * device needed), per stream: a header of 16 words - frames seen (it stops at 2^32 - 1; only the mean's divisor and the EMA's first
 * frame read it), ring position, a ticket word, 0, a magic word, op, k (0 for the EMA), h, w, zeros - and a ring of k - 1 planes of
 * h * w floats padded to 16 bytes (EMA: one plane, y[t-1]).  A call of t frames writes its last min(t, k - 1) frames into the ring;
 * nothing is shifted.  The counters are advanced on the device, so a captured call can be replayed.  vad_tfilt_init writes fresh
 * state for b streams (asynchronous); one stream of a blob is re-initialised by a call with its address (state + s * bytes / b) and
 * b = 1.  A blob that was made for another op, k, h or w is detected on the device: out is NaN and the blob is left alone.
 * VAD_ERR_ARG for an unknown op, k outside 1 .. VAD_TFILT_MAX_K (min, max, mean), alpha not in (0, 1) or NaN (ema), b, t, h, w out
 * of range, a NULL or misaligned pointer, out overlapping maps.  b == 0 or t == 0 returns VAD_OK and launches nothing.  One launch
 * per call (per 65535 streams) on `stream`, one read and one write of the maps plus the ring, no workspace, no allocation, no host
 * synchronisation: capturable in a graph.  16-byte loads and stores when h * w is a multiple of 4 and maps, out are 16-byte
 * aligned; one pixel per work item otherwise.
 * vad_tfilt_plan: the threads of a work-group and the pixels of a work item on the 16-byte path - a stream of more than threads *
 * vector_pixels pixels has more than one work-group on either path. */
#define VAD_TFILT_MAX_K 16
enum { VAD_TFILT_MIN = 0, VAD_TFILT_MAX = 1, VAD_TFILT_MEAN = 2, VAD_TFILT_EMA = 3 };
size_t vad_tfilt_state_bytes(long long b, int h, int w, int op, int k);
int vad_tfilt_init(void* state, long long b, int h, int w, int op, int k, void* stream);
int vad_tfilt_maps(const float* maps, long long b, int t, int h, int w, int op, int k, float alpha, void* state_or_null, float* out,
                   void* stream);
int vad_tfilt_plan(int* threads, int* vector_pixels);

/* ------------------------------------------------------------------ Defect regions of an anomaly map (csrc/map_regions.hip)
 * What turns a map and an operating threshold into detections: the connected regions of {v >= threshold} of every frame, as a
 * compact table - where they are, how large, how strong.  The maps stay on the device; the table is what leaves it.
 *
 * vad_detect_regions: maps = n frames of h x w fp32, contiguous, 4-byte aligned (the limits of vad_label_regions: any h, w >= 1
 * with h * w < 2^31 - 1; n * h * w <= 2^38).  A pixel is foreground iff v >= threshold - the predicate of the ROC thresholds, which
 * apply as they stand; a NaN pixel never is (it is counted, below), +Inf always is; a NaN threshold is refused.  Regions are those
 * of vad_label_regions (the same kernels, the same canonical labels, connectivity 8 or 4, every frame on its own, every walk
 * bounded, the flag word in the first uint32 of ws).  labels_or_null int32 [n, h, w], when given, receives the labels of ALL
 * foreground regions, those dropped for their area included.
 * records uint32 [n, max_regions, VAD_REGION_WORDS], 16-byte aligned; one region is
 *     word 0      root: the smallest y * w + x of the region
 *     word 1      area in pixels
 *     words 2-5   x0, y0, x1, y1 of the bounding box, inclusive
 *     word 6      peak: the float bits of the region's maximum
 *     word 7      peak index: the smallest y * w + x among the pixels that hold the maximum
 *     words 8-9   uint64 sum of x over the region's pixels      (centroid = sum / area, exactly)
 *     words 10-11 uint64 sum of y
 * Values compare through the order-preserving key of their bits, so -0.0 < +0.0.  The regions with area >= min_area (>= 1) are
 * kept, in ascending order of their roots - raster order of their first pixel, scipy.ndimage.label's numbering -, and the first
 * min(kept, max_regions) are written (max_regions in 1 .. 65536); every other record of the frame is all-zero.
 * counts uint32 [n, 4]: kept (the full number, which may exceed max_regions: truncation is visible), dropped for area, foreground
 * pixels, NaN pixels.  Integer atomics, min and max only: both tables are the same words for any batching, launch order or tiling.
 * ws: caller-provided, 16-byte aligned, vad_regions_workspace_bytes(n, h, w, labels_given) bytes (0 for arguments out of range; no
 * device is needed): 16 bytes for the flag word, 4 bytes per chunk of 1024 pixels of every frame (padded to 16), then 4 bytes per
 * pixel each for region sizes and record slots and, with labels_given = 0 (labels_or_null is NULL), for the label plane.
 * VAD_ERR_ARG for a NULL or misaligned pointer, n, h, w out of range, a connectivity other than 4 or 8, min_area == 0, max_regions
 * out of range and a NaN threshold; VAD_ERR_WS for a short workspace.  n == 0 clears the flag word only.  Every launch is
 * asynchronous on `stream`; nothing is allocated, the host never waits, the call can be captured into a graph. */
#define VAD_REGION_WORDS 12
size_t vad_regions_workspace_bytes(long long n, int h, int w, int labels_given);
int vad_detect_regions(const float* maps, long long n, int h, int w, float threshold, int connectivity, unsigned min_area,
                       int max_regions, int32_t* labels_or_null, uint32_t* records /* [n, max_regions, 12] */,
                       uint32_t* counts /* [n, 4] */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ Detections against ground-truth masks (csrc/map_match.hip)
 * What an operating point is accepted on: how many of the labelled defects it finds, how many false alarms it raises, which pixel
 * IoU it reaches.  The regions of vad_detect_regions joined with the regions of the frame's mask; maps, masks and both labellings
 * stay on the device.  Everything is an integer, per frame.
 *
 * vad_match_regions: maps = n frames of h x w fp32, contiguous, 4-byte aligned; masks = n x h x w elements in mask_format -
 * VAD_LBL_U8_ELEM (anomalous iff >= 128) or VAD_LBL_F32_ELEM (iff > 0.5; 4-byte aligned) - with the limits of vad_label_regions.
 * Predicted foreground is v >= threshold exactly as in vad_detect_regions (a NaN pixel never is and is counted, +Inf always is, a
 * NaN threshold is refused); its connected regions (connectivity 8 or 4) with area >= min_area (>= 1) are KEPT, and P is the set of
 * their pixels: a region dropped for its area contributes nothing, its pixels count as background everywhere below.  G is the set
 * of the mask's anomalous pixels; its connected regions under the same connectivity all count.
 *     a mask region g       hit(g) = |g & P|;      DETECTED iff hit >= 1     and (double)hit     >= gt_fraction   * (double)area
 *     a kept prediction p   overlap(p) = |p & G|;  MATCHED  iff overlap >= 1 and (double)overlap >= pred_fraction * (double)area
 * - one IEEE double multiply and one compare, no fused multiply-add, no division: numpy float64 restates it bit for bit.  Both
 * fractions are doubles in [0, 1]; 0 means "any shared pixel".  Overlap is shared pixels: adjacency, diagonal too, is none.  A
 * kept prediction that is not matched is a false alarm.
 * gt_records, pred_records uint32 [n, max_regions, VAD_MATCH_WORDS], 16-byte aligned; one region is
 *     word 0   root: the smallest y * w + x of the region
 *     word 1   area in pixels
 *     word 2   hit (gt_records) or overlap (pred_records)
 *     word 3   flags: bit 0 = detected (gt_records) or matched (pred_records)
 * gt_records holds the frame's mask regions, pred_records its kept predictions, both in ascending order of their roots - raster
 * order of their first pixel, scipy.ndimage.label's numbering; the first min(count, max_regions) are written (max_regions in
 * 1 .. 65536), every other record is all-zero.  pred_records words 0-1 are vad_detect_regions' words 0-1 for the same arguments,
 * gt_records words 0-1 the roots and sizes of vad_label_regions.
 * counts uint64 [n, VAD_MATCH_COUNTS], 8-byte aligned, per frame:
 *     words 0-1    mask regions; detected mask regions
 *     words 2-4    kept predictions; matched predictions; false alarms (word 2 - word 3)
 *     word 5       predictions dropped for their area
 *     words 6-9    pixels of P & G (true positives), of P \ G (false positives), of G \ P (false negatives), of neither
 *     word 10      NaN pixels of the map (they fall into words 8 or 9 by their mask)
 *     word 11      |G|
 *     words 12-15  the frame's class, one-hot: mask regions and kept predictions; no mask region but kept predictions; mask regions
 *                  but no kept prediction; neither
 * The region counters are the full numbers, which may exceed max_regions: truncation is visible.  Every word sums over frames; the
 * sum of words 12-15 is the number of frames.  Integer atomics only: all three outputs are the same words for any batching, launch
 * order or tiling.
 * ws: caller-provided, 16-byte aligned, vad_match_workspace_bytes(n, h, w) bytes (0 for arguments out of range; no device is
 * needed): 16 bytes for the flag word - the first uint32; the second uint32 is what the labelling of the masks reported, folded
 * into the first -, 8 bytes per chunk of 1024 pixels of every frame (two chunk counters; padded to 16), then 24 bytes per pixel:
 * 4 each for the two label planes, the two size planes and the per-root hit and overlap planes.  Every walk of the union-find is
 * bounded as in vad_label_regions; one that runs out of its budget sets bit 0 of the flag word.
 * vad_match_plan reports the pixels of a frame that one grid round of each pass covers (the labeller, the join, the count / slot
 * scan) and the threads of a work-group - what a test needs to build a frame larger than one round of every pass.
 * VAD_ERR_ARG for a NULL or misaligned pointer, an unknown mask_format, n, h, w out of range, a connectivity other than 4 or 8,
 * min_area == 0, max_regions out of range, a NaN threshold and a fraction that is NaN or outside [0, 1]; VAD_ERR_WS for a short
 * workspace.  n == 0 clears the flag word only.  Every launch is asynchronous on `stream`; nothing is allocated, the host never
 * waits, the call can be captured into a graph. */
#define VAD_MATCH_WORDS 4
#define VAD_MATCH_COUNTS 16
size_t vad_match_workspace_bytes(long long n, int h, int w);
int vad_match_regions(const float* maps, const void* masks, int mask_format, long long n, int h, int w, float threshold,
                      int connectivity, unsigned min_area, double gt_fraction, double pred_fraction, int max_regions,
                      uint32_t* gt_records /* [n, max_regions, 4] */, uint32_t* pred_records /* [n, max_regions, 4] */,
                      uint64_t* counts /* [n, 16] */, void* ws, size_t ws_bytes, void* stream);
int vad_match_plan(int* label_round, int* join_round, int* scan_round, int* threads);

/* ------------------------------------------------------------------ Anomaly events of a clip (csrc/map_events.hip)
 * Regions linked across the frames of a clip: an event is a connected component of {v >= threshold} in the volume [t, h, w] of one
 * clip.  The predicate is the one of vad_detect_regions (a NaN pixel never is foreground and is counted, +Inf always is, a NaN
 * threshold is refused).  Inside a frame pixels connect as there (connectivity 8 or 4); between consecutive frames
 *     temporal 1   (t, y, x) links to (t-1, y, x)
 *     temporal 9   (t, y, x) links to every foreground pixel of the 3 x 3 around (y, x) in frame t-1; connectivity 8 only
 * so (4, 1), (8, 1) and (8, 9) are scipy.ndimage.label's 6-structure, its 3 x 3 centre plane with single-pixel outer planes, and
 * its 26-structure.  Frames of different clips never link, nor do rows of different frames.  An event has no gaps in time.
 *
 * vad_detect_events: maps = b clips of t frames of h x w fp32, contiguous, 4-byte aligned; h, w, t >= 1, t * h * w < 2^31 - 1 (a
 * volume index fits the int32 label plane), b * t * h * w <= 2^38.  The root of an event is the smallest volume index
 * t * h * w + y * w + x of its pixels.  labels_or_null int32 [b, t, h, w], when given, receives 0 or 1 + root for every foreground
 * pixel, whether its event passes the filters or not.
 * records uint32 [b, max_events, VAD_EVENT_WORDS], 16-byte aligned; one event is
 *     word 0       root
 *     word 1       volume in pixels
 *     words 2-3    t0, t1: first and last frame, inclusive
 *     words 4-7    x0, y0, x1, y1 of the union of its frames' boxes, inclusive
 *     word 8       peak: the float bits of the event's maximum
 *     word 9       peak index: the smallest volume index among the pixels that hold the maximum
 *     words 10-11  uint64 sum of x over the event's pixels      (centroid = sum / volume, exactly)
 *     words 12-13  uint64 sum of y
 *     words 14-15  uint64 sum of t
 * Values compare through the order-preserving key of their bits, so -0.0 < +0.0.  The events with t1 - t0 + 1 >= min_duration
 * (>= 1) and volume >= min_volume (>= 1) are kept, in ascending order of their roots - scipy.ndimage.label's numbering of a 3-D
 * array -, and the first min(kept, max_events) are written (max_events in 1 .. 65536); every other record of the clip is all-zero.
 * counts uint32 [b, 4]: kept (the full number, which may exceed max_events), dropped by a filter, foreground pixels, NaN pixels.
 * frame_counts uint32 [b, t, 3]: foreground pixels of the frame, pixels of the frame that belong to KEPT events (whether or not
 * the event has a record: the word does not depend on max_events; the frame alarms iff it is non-zero), NaN pixels of the frame.
 * Integer atomics, min and max only: every output is the same words for any batching of clips, launch order or tiling.
 * Every walk of the union-find is bounded by a number known at launch (2 * t * h * w + 2 steps); one that runs out of it sets the
 * flag word - the first uint32 of ws - and leaves.
 * ws: caller-provided, 16-byte aligned, vad_events_workspace_bytes(b, t, h, w, labels_given) bytes (0 for arguments out of range;
 * no device is needed): 16 bytes for the flag word, 4 bytes per chunk of 1024 pixels of every clip (padded to 16), then 4 bytes
 * per pixel each for event sizes and for last frames / record slots and, with labels_given = 0, for the label plane.
 * vad_events_plan reports the pixels one grid round of each pass covers (the labeller inside a frame; rebase, link and flatten
 * over a clip's volume; the count / slot scan; the reduction) and the threads of a work-group - what a test needs to build a
 * volume that is larger than one round of every pass.
 * VAD_ERR_ARG for a NULL or misaligned pointer, b, t, h, w out of range, a connectivity other than 4 or 8, a temporal other than 1
 * or 9, temporal 9 with connectivity 4, min_duration == 0, min_volume == 0, max_events out of range and a NaN threshold;
 * VAD_ERR_WS for a short workspace.  b == 0 clears the flag word only.  Every launch is asynchronous on `stream`; nothing is
 * allocated, the host never waits, the call can be captured into a graph. */
#define VAD_EVENT_WORDS 16
size_t vad_events_workspace_bytes(long long b, int t, int h, int w, int labels_given);
int vad_detect_events(const float* maps, long long b, int t, int h, int w, float threshold, int connectivity, int temporal,
                      unsigned min_duration, unsigned min_volume, int max_events, int32_t* labels_or_null,
                      uint32_t* records /* [b, max_events, 16] */, uint32_t* counts /* [b, 4] */,
                      uint32_t* frame_counts /* [b, t, 3] */, void* ws, size_t ws_bytes, void* stream);
int vad_events_plan(int* label_round, int* volume_round, int* scan_round, int* reduce_round, int* threads);

/* ------------------------------------------------------------------ Events against ground-truth masks (csrc/map_event_match.hip)
 * What a debounced alarm is accepted on: how many of the labelled anomalies it still finds, how many false-alarm events it raises,
 * how many frames after a defect appears it fires.  The kept events of vad_detect_events joined with the connected tracks of the
 * clip's mask volume - vad_match_regions in three dimensions; maps, masks and both labellings stay on the device.  Everything is an
 * integer, per clip.
 *
 * vad_match_events: maps = b clips of t frames of h x w fp32 with the limits of vad_detect_events; masks = b x t x h x w elements
 * in mask_format - VAD_LBL_U8_ELEM (anomalous iff >= 128) or VAD_LBL_F32_ELEM (iff > 0.5; 4-byte aligned).  The predictions are the
 * events of vad_detect_events for the same threshold, connectivity and temporal (foreground is v >= threshold; a NaN voxel never is
 * and is counted); those that pass min_duration and min_volume are KEPT, and P is the set of their voxels: a dropped event
 * contributes nothing, its voxels count as background everywhere below.  G is the set of the masks' anomalous voxels; its connected
 * components under the same (connectivity, temporal) structure are the ground-truth TRACKS, and all of them count.  Clips never
 * link.
 *     a track g        hit(g) = |g & P|;      DETECTED iff hit >= 1     and (double)hit     >= gt_fraction   * (double)volume
 *     a kept event p   overlap(p) = |p & G|;  MATCHED  iff overlap >= 1 and (double)overlap >= pred_fraction * (double)volume
 * - one IEEE double multiply and one compare, no fused multiply-add, no division, as in vad_match_regions.  Overlap is shared
 * voxels: adjacency in space or in time is none.  A kept event that is not matched is a false alarm.  The DELAY of a detected track
 * is the first frame of a shared voxel minus the track's first frame.
 * gt_records, pred_records uint32 [b, max_events, VAD_EVMATCH_WORDS], 16-byte aligned; one track or event is
 *     word 0       root: the smallest volume index t * h * w + y * w + x
 *     word 1       volume in voxels
 *     words 2-3    t0, t1: first and last frame, inclusive
 *     word 4       hit (gt_records) or overlap (pred_records)
 *     words 5-6    first and last frame of a shared voxel; both 0xffffffff when word 4 is 0
 *     word 7       flags: bit 0 = detected (gt_records) or matched (pred_records)
 * both in ascending order of their roots - scipy.ndimage.label's numbering of a 3-D array; the first min(count, max_events) are
 * written (max_events in 1 .. 65536), every other record is all-zero.  pred_records words 0-3 are vad_detect_events' words 0-3 for
 * the same arguments.
 * counts uint64 [b, VAD_EVMATCH_COUNTS], 8-byte aligned, per clip:
 *     words 0-1    tracks; detected tracks
 *     words 2-4    kept events; matched events; false-alarm events (word 2 - word 3)
 *     word 5       events dropped by a filter
 *     words 6-9    voxels of P & G, of P \ G, of G \ P, of neither
 *     word 10      NaN voxels of the maps (they fall into words 8 or 9 by their mask)
 *     word 11      |G|
 *     word 12      the sum of the delays of the detected tracks
 *     word 13      detected tracks with delay 0
 *     words 14-17  frames with voxels of G and of P; of P only (false-alarm frames); of G only (missed frames); of neither
 *     words 18-21  the clip's class, one-hot: tracks and kept events; kept events only; tracks only; neither
 * The track and event counters are the full numbers, which may exceed max_events: truncation is visible.  Every word sums over
 * clips, batches and ranks.
 * frame_counts uint32 [b, t, 4], 4-byte aligned: voxels of P & G, of P \ G, of G \ P and NaN voxels of the frame; word 0 + word 1
 * is vad_detect_events' frame_counts word 1.
 * Integer atomics, min and max only: all four outputs are the same words for any batching of clips, launch order or tiling.  Every
 * walk of the union-find is bounded as in vad_detect_events; one that runs out of its budget sets bit 0 of the flag word.
 * ws: caller-provided, 16-byte aligned, vad_event_match_workspace_bytes(b, t, h, w) bytes (0 for arguments out of range; no device
 * is needed): 16 bytes for the flag word - the first uint32; the second uint32 is what the in-frame labelling of the masks
 * reported, folded into the first -, 4 bytes per chunk of 1024 voxels of every clip for the events and again for the tracks (each
 * padded to 16), then 48 bytes per voxel: 4 each for labels, sizes and last frames of the events, the same three of the tracks,
 * then hit, first and last shared frame at the tracks' roots and overlap, first and last shared frame at the events' roots.
 * vad_event_match_plan reports the pixels one grid round of each pass covers (the labeller inside a frame; rebase, link, flatten
 * and init over a clip's volume; the count / slot scan; the join) and the threads of a work-group.
 * VAD_ERR_ARG for what vad_detect_events refuses, an unknown mask_format, misaligned float masks and a fraction that is NaN or
 * outside [0, 1]; VAD_ERR_WS for a short workspace.  b == 0 clears the flag word only.  Every launch is asynchronous on `stream`;
 * nothing is allocated, the host never waits, the call can be captured into a graph. */
#define VAD_EVMATCH_WORDS 8
#define VAD_EVMATCH_COUNTS 22
size_t vad_event_match_workspace_bytes(long long b, int t, int h, int w);
int vad_event_match_plan(int* label_round, int* volume_round, int* scan_round, int* join_round, int* threads);
int vad_match_events(const float* maps, const void* masks, int mask_format, long long b, int t, int h, int w, float threshold,
                     int connectivity, int temporal, unsigned min_duration, unsigned min_volume, double gt_fraction,
                     double pred_fraction, int max_events, uint32_t* gt_records /* [b, max_events, 8] */,
                     uint32_t* pred_records /* [b, max_events, 8] */, uint64_t* counts /* [b, 22] */,
                     uint32_t* frame_counts /* [b, t, 4] */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ Anomaly events across the calls of a live stream (csrc/map_track.hip)
 * The events of vad_detect_events, continued frame by frame: a stream is the sequence of its maps [h, w] since the last init, an
 * event a connected component of {v >= threshold} in the stream's volume so far - same predicate, same three structures
 * (connectivity, temporal) = (4, 1), (8, 1), (8, 9).  The frame numbers t = 0, 1, ... are counted on the device, in the state: the
 * host passes none, so a captured call can be replayed.  After frame t an event is OPEN iff it has a pixel in frame t; it CLOSES at
 * the arrival of frame t1 + 1 when no pixel of that frame links to it.  Two open events joined by a region of the new frame are one
 * from then on (root: the smaller (t0, root pixel); sums, volume and box combined); a split leaves one event; an event absent for
 * one frame closes and a new one begins.  Streams never link.
 *
 * One record is VAD_TRACK_WORDS = 20 uint32 words (80 bytes, 16-byte aligned):
 *     word 0       root_pixel: y * w + x of the smallest pixel of the event's first frame (root = t0 * h * w + root_pixel)
 *     words 1-2    t0, t1: first and last frame, inclusive
 *     word 3       handle: the smallest pixel of the event in frame t1
 *     words 4-7    x0, y0, x1, y1 of the union of its frames' boxes, inclusive
 *     word 8       peak: the float bits of the event's maximum (order key of vad_detect_regions: -0.0 < +0.0)
 *     words 9-10   peak_pixel, peak_frame: among the pixels that hold the maximum the earliest frame, then the smallest pixel
 *     word 11      reserved, zero
 *     words 12-13  uint64 volume in pixels (an all-foreground 256 x 256 stream passes 2^32 pixels in 36 minutes at 30 frames/s)
 *     words 14-15  uint64 sum of x             (centroid = sum / volume, exactly)
 *     words 16-17  uint64 sum of y
 *     words 18-19  uint64 sum of t, exact modulo 2^64: it wraps once h * w * T * (T - 1) / 2 of an always-foreground stream reaches
 *                  2^64 - at 256 x 256 from T = 23.7 million frames on (nine days at 30 frames/s), at 2^24 pixels from 1.48 million
 *
 * State (caller-owned device memory, 16-byte aligned, vad_track_state_bytes(b, h, w, max_open) bytes; 0 for arguments out of range,
 * no device needed), per stream: a header of 16 words - frames seen, open events, events lost in total (sticky), flags (sticky:
 * VAD_LABEL flag bit 0 = a walk ran out of its budget, VAD_TRACK_FLAG_COUNTER = the frame counter stands at 2^32 - 1 and no longer
 * advances), a magic word, h, w, max_open, zeros -, the open table [max_open, 20] (slot r = the open event whose handle has rank r
 * in raster order; all-zero records behind the open ones), the slot plane [h * w] of the newest frame (0, slot + 1, or 0xffffffff
 * for an open event without a record), padded to 16 bytes.  vad_track_init writes a fresh header, table and plane (asynchronous).
 * max_open in 1 .. 65536: an open event of rank >= max_open has no record; it is counted as LOST, once, in counts and in the
 * header; its pixels never alarm and count as background for the links of the next frame.  Visible, never silent.
 *
 * vad_track_events continues b streams by t >= 1 maps each (maps fp32 [b, t, h, w], contiguous, 4-byte aligned; h * w <= 2^24,
 * b <= 2^20, b * t * h * w <= 2^38):
 * closed uint32 [b, max_closed, 20], 16-byte aligned: the events that closed in this call and pass t1 - t0 + 1 >= min_duration and
 *     volume >= min_volume with their final values, in ascending (t1, handle) order - the same for any split of the frames over
 *     calls -, the first min(kept, max_closed) written (max_closed in 1 .. 65536), every other record all-zero.
 * counts uint32 [b, 6]: closed and kept (the full number), closed and dropped by a filter, foreground pixels, NaN pixels, events
 *     open after the call, events lost in this call.
 * frame_counts uint32 [b, t, 3]: foreground pixels of the frame; pixels of the frame that belong to events which alarm NOW
 *     (t - t0 + 1 >= min_duration and the volume so far >= min_volume: the causal counterpart of vad_detect_events' word,
 *     independent of max_closed); NaN pixels of the frame.
 * vad_track_flush closes every open event as if an empty frame had arrived, without advancing the counter, in slot order through
 * the same filters; the table and the plane are zero afterwards.  Its ws is vad_track_workspace_bytes(b, 0, h, w, max_open).
 * ws: caller-provided, 16-byte aligned, vad_track_workspace_bytes(b, t, h, w, max_open) bytes (0 out of range, no device needed):
 * 16 bytes for the flag word (its first uint32: cleared by every call, set by a walk out of budget or the counter's end), then -
 * each padded to 16 - the labels 4 * b * t * h * w, 4 * b * max_open, 4 per chunk of 1024 pixels of a frame and stream, 4 * b * h * w,
 * the working records 96 * b * max_open, 4 * b.
 * vad_track_plan: the pixels one grid round covers in the labeller, in the link / reduce passes, in the flatten / slot scan, the
 * slots one round of the table passes covers, and the threads of a work-group.
 * Integer atomics, min and max only: every output, the table and the plane are the same words for any batching of streams and any
 * split of the frames over calls.  VAD_ERR_ARG for a NULL or misaligned pointer, b, t, h, w out of range, a connectivity other than
 * 4 or 8, a temporal other than 1 or 9, temporal 9 with connectivity 4, min_duration == 0, min_volume == 0, max_open or max_closed
 * out of range and a NaN threshold; VAD_ERR_WS for a short workspace.  Every launch is asynchronous on `stream`; nothing is
 * allocated, the host never waits; a call with fixed t can be captured into a graph. */
#define VAD_TRACK_WORDS 20
#define VAD_TRACK_FLAG_COUNTER 4u
size_t vad_track_state_bytes(long long b, int h, int w, int max_open);
size_t vad_track_workspace_bytes(long long b, int t, int h, int w, int max_open);
int vad_track_init(void* state, long long b, int h, int w, int max_open, void* stream);
int vad_track_events(const float* maps, long long b, int t, int h, int w, float threshold, int connectivity, int temporal,
                     unsigned min_duration, unsigned min_volume, int max_open, int max_closed, void* state,
                     uint32_t* closed /* [b, max_closed, 20] */, uint32_t* counts /* [b, 6] */,
                     uint32_t* frame_counts /* [b, t, 3] */, void* ws, size_t ws_bytes, void* stream);
int vad_track_flush(long long b, int h, int w, unsigned min_duration, unsigned min_volume, int max_open, int max_closed, void* state,
                    uint32_t* closed /* [b, max_closed, 20] */, uint32_t* counts /* [b, 6] */, void* ws, size_t ws_bytes, void* stream);
int vad_track_plan(int* label_round, int* pixel_round, int* scan_round, int* table_round, int* threads);

/* ------------------------------------------------------------------ Per-frame tracks of anomaly events (csrc/map_event_tracks.hip)
 * A box per event and frame, where the event tables above hold the union box of an event's whole life.  A CROSS-SECTION is the set
 * of one event's pixels in one frame; it is one record of VAD_REGION_WORDS = 12 uint32 words in the layout of vad_detect_regions,
 * so whatever reads a region record reads it:
 *     word 0      the smallest y * w + x of the event's pixels in this frame
 *     word 1      area: the event's pixels in this frame
 *     words 2-5   x0, y0, x1, y1 of their bounding box, inclusive
 *     word 6      peak: the float bits of the maximum over these pixels
 *     word 7      peak index: the smallest y * w + x among the pixels that hold the maximum
 *     words 8-9   uint64 sum of x over these pixels             (centroid = sum / area, exactly)
 *     words 10-11 uint64 sum of y
 * Values compare through the order-preserving key of their bits, so -0.0 < +0.0.  A cross-section may be disconnected inside its
 * frame - its pieces may join through other frames - and is still ONE record; a frame in which the event has no pixel is an
 * all-zero record.
 *
 * vad_event_tracks (a clip): maps fp32 [b, t, h, w] and labels int32 [b, t, h, w], records uint32 [b, max_events, VAD_EVENT_WORDS]
 * and counts uint32 [b, 4] as ONE vad_detect_events call took and wrote them (labels: 0 or 1 + root; the kept records of a clip are
 * its first min(counts[.][0], max_events), their roots ascend), with that call's limits on b, t, h, w and max_events in 1 .. 65536.
 * tracks uint32 [b, max_events, t, 12], 16-byte aligned, event-major - one event's track is 48 * t contiguous bytes -, at most
 * b * max_events * t = 2^26 records (3 GiB).  Record (e, f) is the cross-section of kept event e in frame f; the records of the
 * slots behind the kept ones are all-zero; pixels of events that a filter dropped, or that have no record because the table was
 * truncated, contribute nothing.  A pixel's record is found by its root, once per distinct root of a wave.  Three launches.
 * vad_event_tracks_plan reports the pixels of a clip one grid round of the reduction covers and the threads of a work-group.
 *
 * vad_track_boxes (a live stream): after vad_track_events the state holds the open table and the slot plane of the newest frame.
 * maps_newest fp32: the newest map [h, w] of stream s begins at maps_newest + s * frame_stride (frame_stride in floats, >= h * w:
 * the last frame of a [b, t, h, w] call is used in place with maps + (t - 1) * h * w and frame_stride t * h * w); b, h, w, max_open
 * with the limits of vad_track_events.  boxes uint32 [b, max_open, 12], 16-byte aligned: record r is the cross-section in the
 * newest frame of the open event in slot r - its word 0 is that event's handle, word 3 of its open record -, all-zero behind the
 * open ones; pixels of a lost event (0xffffffff in the plane) contribute nothing.  The header's magic, h, w and max_open are
 * compared ON THE DEVICE: with any other blob every record is zero and nothing of the blob beyond its header is read.
 *
 * Integer atomics, min and max only: both tables are the same words for any batching, launch order or tiling.  No workspace, no
 * flag word (there is no union-find walk), no host read.  VAD_ERR_ARG for a NULL or misaligned pointer, b, t, h, w out of range,
 * max_events or max_open out of range, more than 2^26 records, a frame_stride below h * w.  b == 0 launches nothing.  Every launch
 * is asynchronous on `stream`; nothing is allocated, the host never waits, the calls can be captured into a graph. */
int vad_event_tracks(const float* maps, const int32_t* labels, const uint32_t* records /* [b, max_events, 16] */,
                     const uint32_t* counts /* [b, 4] */, long long b, int t, int h, int w, int max_events,
                     uint32_t* tracks /* [b, max_events, t, 12] */, void* stream);
int vad_event_tracks_plan(int* reduce_round, int* threads);
int vad_track_boxes(const float* maps_newest, long long frame_stride, long long b, int h, int w, int max_open, const void* state,
                    uint32_t* boxes /* [b, max_open, 12] */, void* stream);

/* ------------------------------------------------------------------ Per-pixel calibration of anomaly maps (csrc/map_stats.hip)
 * The mean and standard deviation of every pixel of the anomaly map over the normal (training) frames, and the z-score map
 * z = (map - mean) / std that is ranked, thresholded and labelled in place of the raw map.  The maps stay on the device.
 *
 * State blob (caller-owned device memory, 16-byte aligned, vad_mapstat_state_bytes(h, w) bytes; 0 for h, w below 1 or h * w above
 * VAD_MAX_FRAME_PIXELS, no device needed):
 *     uint32 magic "VADM", abi << 16;  int32 h, w;  uint64 n (frames seen), uint64 reserved;  float64 K[h*w], S1[h*w], S2[h*w]
 * vad_mapstat_reset writes the header and zeroes the planes.  The count lives on the device, so every call below is asynchronous
 * on `stream`, allocates nothing, never waits for the device and can be captured into a graph; a replayed accumulate accumulates
 * again.  The header is compared with the call's h, w ON THE DEVICE (the host cannot see it without waiting): with a blob made
 * for another geometry, or not a state, accumulate and merge change nothing and follow no offset of it, and finalize writes NaN.
 *
 * Arithmetic, float64, every operation rounded on its own (no fused multiply-add), so numpy restates it bit for bit and a result
 * does not depend on how the frames were batched:
 * vad_mapstat_accumulate: maps = n frames of h x w fp32, contiguous, 4-byte aligned.  Per pixel, in frame order: if the state is
 *   empty K = (double)x[0]; for every frame d = (double)x - K, S1 = S1 + d, S2 = S2 + d * d; then n grows by the call's n.  One
 *   thread owns a pixel (its additions are never split), with vad_mapstat_plan's frames_in_flight loads outstanding.  A NaN, or an
 *   Inf in the first frame, makes the pixel's mean and std NaN; a later Inf makes its std NaN and its mean that infinity; no
 *   other pixel changes a bit.  Two launches (the pixels, then the count).
 * vad_mapstat_merge: state += other (two launches).  dl = K_b - K_a; S1 = S1_a + (S1_b + n_b dl); S2 = S2_a + (S2_b + ((2 dl) S1_b +
 *   (n_b dl) dl)), evaluated in that order; the counts are added and K_a is kept; if either side is empty the result is the other.
 * vad_mapstat_finalize: mean, std fp32 [h*w] (either may be NULL, not both).  mean = fl32(K + S1 / n); var = (S2 - S1 (S1 / n)) /
 *   (n - ddof), var < 0 -> 0 (a NaN stays), std = sqrtf(fl32(var)): the root in fp32, correctly rounded.  ddof is 0 or 1.  With
 *   n == 0 both are NaN everywhere, with n - ddof <= 0 std is.  One launch.
 * vad_map_normalize: z = (x - mean) / den, den = std < min_std ? min_std : std (a NaN std stays NaN), fp32, each operation rounded
 *   on its own, IEEE division; min_std finite and > 0.  out (may be NULL) may be maps itself - in place - but must not partly
 *   overlap it.  frame_max (may be NULL; not both): [n], the maximum of each normalised frame with torch.amax semantics,
 *   compare-only: the same for every batching and tiling.  ws: vad_map_normalize_workspace_bytes(n, h, w) bytes (0 for arguments
 *   out of range), needed only with frame_max.  One launch (two with frame_max).
 * vad_mapstat_plan reports pixels per thread, frames in flight per thread and threads per work-group of the accumulate kernel -
 *   what a test needs to build shapes that cross its internal boundaries.
 * VAD_ERR_ARG for h, w below 1 or h * w above VAD_MAX_FRAME_PIXELS, n < 0, a NULL or misaligned pointer (states 16 bytes, the rest 4),
 * other overlapping state, ddof outside 0..1, a min_std that is not finite and > 0, both outputs NULL, a partly overlapping out;
 * VAD_ERR_WS for a short workspace.  n == 0 returns VAD_OK and launches nothing. */
size_t vad_mapstat_state_bytes(int h, int w);
int vad_mapstat_reset(void* state, int h, int w, void* stream);
int vad_mapstat_accumulate(const float* maps, long long n, int h, int w, void* state, void* stream);
int vad_mapstat_merge(void* state, const void* other, int h, int w, void* stream);
int vad_mapstat_finalize(const void* state, int h, int w, int ddof, float* mean, float* std_out, void* stream);
size_t vad_map_normalize_workspace_bytes(long long n, int h, int w);
int vad_map_normalize(const float* maps, long long n, int h, int w, const float* mean, const float* std_in, float min_std, float* out,
                      float* frame_max, void* ws, size_t ws_bytes, void* stream);
int vad_mapstat_plan(int* pixels_per_thread, int* frames_in_flight, int* threads);

/* ------------------------------------------------------------------ hipGraph capture / replay of a scoring call
 * vad_graph_begin(stream); <one vad_img_score* / vad_vid_score* call on `stream`>; vad_graph_end(stream, &exec) captures
 * the call's launch sequence (kernels, and the fork / join with the library's helper streams) into an instantiated
 * hipGraph; vad_graph_launch(exec, stream) replays it asynchronously with the SAME device pointers (keep input, output and
 * workspace buffers alive and write new frames into the same input buffer).  Run the call once eagerly first: the first
 * call of a thread creates helper streams and queries occupancy, which must not happen inside a capture.  Per-layer timing
 * is skipped while capturing.  Results are bit-identical to the eager call. */
int vad_graph_begin(void* stream);
int vad_graph_end(void* stream, void** exec_out);
int vad_graph_launch(void* exec, void* stream);
int vad_graph_destroy(void* exec);

/* ------------------------------------------------------------------ per-layer timing
 * When enabled, the model-level calls bracket every layer launch with hipEvents on `stream`.
 * vad_prof_read synchronises the events and returns the accumulated ms and launch count per
 * layer slot since the last vad_prof_reset.  The record list is mutex-guarded: threads may score concurrently while
 * profiling is on (their records are pooled). */
#define VAD_PROF_SLOTS 32
int vad_prof_enable(int on);
int vad_prof_reset(void);
int vad_prof_read(float* ms /*[VAD_PROF_SLOTS]*/, int* launches /*[VAD_PROF_SLOTS]*/);
const char* vad_prof_slot_name(int model /*0 img, 1 vid, 2 video training step (kernel groups)*/, int slot);

#ifdef __cplusplus
}
#endif
#endif
