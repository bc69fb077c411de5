/*
 * dasr.h — C ABI of the MI355X-native DepthNet hot path (libdasr_hip.so).
 *
 * The reference (CUHK-AIM-Group/Depth-Aware-Endoscopy-SR) is pure Python: the generator
 * DepthNet (codes/models/modules/sftmd_arch.py:837-950) and its SEAN/DFN normalisation
 * (codes/models/modules/normalization.py:7-92) dispatch every device op through torch.nn
 * (cuDNN/cuBLAS/ATen). It has no FFI of its own; these entry points are what a binding
 * for this path replaces, one per group of torch ops, each citing the reference lines.
 * INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes, no torch types; every pointer is DEVICE memory (HBM),
 *     fp32 unless stated; the caller owns all buffers (outputs and workspaces included).
 *   - activations are NHWC  [B][H][W][C]  (C fastest); the NCHW tensors of the reference
 *     API (input image, depth masks, output image) are converted at the edge by
 *     dasr_nchw_to_nhwc / dasr_clamp_to_nchw or read in place (masks).
 *   - convolution kernels are packed by dasr_weight_pack_fwd into 2*KH*KW*Cin*Cout floats: "HWIO"
 *     [KH][KW][Cin][Cout] followed by the per-tap transpose [KH][KW][Cout][Cin] (so that forward and
 *     data-gradient kernels both stream their K axis contiguously).  Every `w_hwio` argument of the
 *     convolution entry points is such a packed buffer; weight GRADIENTS (dw_hwio) are plain HWIO.
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it, never
 *     synchronise, never allocate, never throw.  Re-entrant: no global mutable state.
 *   - return value: 0 on success, a DASR_E_* code (<0) for bad arguments, or a positive
 *     hipError_t from the launch.  dasr_error_string() names the DASR_E_* codes.
 */
#ifndef DASR_H
#define DASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DASR_OK 0
#define DASR_E_NULL (-1)        /* a required pointer is NULL                         */
#define DASR_E_SHAPE (-2)       /* sizes inconsistent with each other or non-positive  */
#define DASR_E_UNSUPPORTED (-3) /* valid request this build has no kernel for          */
#define DASR_E_WORKSPACE (-4)   /* workspace too small                                 */

/* activation / epilogue selectors for the convolution entry points */
#define DASR_ACT_NONE 0
#define DASR_ACT_RELU 1
#define DASR_ACT_LRELU02 2 /* LeakyReLU(0.2): sftmd_arch.py:741,861-866,891-908 */

int dasr_version(void);
const char* dasr_error_string(int code);
/* 1 when the library was built for the GPU (gfx950), 0 for the CPU kernel emulator used by unit tests */
int dasr_is_device_build(void);

/* ---- layout at the API edge ------------------------------------------------------------ */
/* [B,C,H,W] -> [B,H,W,C]; replaces nothing in the reference (it is NCHW throughout). */
int dasr_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, void* stream);
int dasr_nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, void* stream);
/* torch.clamp(out, min, max) (sftmd_arch.py:950) fused with the NHWC->NCHW edge conversion. */
int dasr_clamp_to_nchw(const float* y_nhwc, float* out_nchw, int B, int C, int H, int W, float lo, float hi,
                       void* stream);
/* backward of the above: dy = dout where lo <= y <= hi, else 0. */
int dasr_clamp_to_nchw_bwd(const float* dout_nchw, const float* y_nhwc, float* dy_nhwc, int B, int C, int H, int W,
                           float lo, float hi, void* stream);
/* F.interpolate(mode='nearest') of an NCHW tensor (normalization.py:58-59). */
int dasr_resize_nearest_nchw(const float* src, float* dst, int BC, int h, int w, int H, int W, void* stream);
/* The same index map applied to the region bytes [B,h,w] -> [B,H,W] of one-hot masks (nearest resize of the K planes
 * == one-hot of the resized region byte): SEAN's mask resize (normalization.py:59) without touching the planes. */
int dasr_resize_nearest_u8(const unsigned char* src, unsigned char* dst, int B, int h, int w, int H, int W,
                           void* stream);

/* ---- weights -------------------------------------------------------------------------------
 * torch.nn.utils.weight_norm, dim 0 (sftmd_arch.py:741,851 and every wn(...) site):
 *   w = g * v / ||v||  with the norm over all dims but 0.
 * v is [O][I][KH][KW] for Conv2d, [I][O][KH][KW] for ConvTranspose2d (transposed=1: dim 0 is the
 * IN-channel axis, encoder.layer4).  g == NULL packs a plain weight (no normalisation).
 * Output: w_hwio = [KH][KW][I][ldo] then [KH][KW][ldo][I] (2*KH*KW*I*ldo floats), written at output-channel offset o_off (ldo >= o_off + O lets several
 * modules share one packed kernel: mlp_gamma_o | mlp_beta_o, normalization.py:41-42, run as one 2C->2C conv);
 * inv_norm [O or I] (1/||v||, kept for the backward; may be NULL when g is).
 */
int dasr_weight_pack_fwd(const float* v, const float* g, float* w_hwio, float* inv_norm, int O, int I, int KH, int KW,
                         int transposed, int ldo, int o_off, void* stream);
/* Every kernel of a network in one launch (a training step re-packs ~120 weight tensors: one launch instead of ~120).
 * One job = one dasr_weight_pack_fwd call; `jobs_host` and `jobs_device` hold the same njobs entries in host / device memory
 * (the host copy is validated, the kernel reads the device copy; the caller keeps both alive until the launch has run).
 *   w, bf16   : the packed kernel, float (bf16 = 0) or bf16 bits (bf16 = 1, as dasr_weight_pack_fwd_bf16)
 *   KK        : KH * KW
 *   amax      : NULL, or an amax buffer (DASR_AMAX_FLOATS floats, see "amax buffers" below) of the packed kernel: the job's norm
 *               groups leave their max |w| in parts o_off .. o_off + O - 1 and the part count ldo (so that jobs sharing one
 *               packed kernel fill one buffer) - what dasr_conv3x3_split2_weights / the 9x9 split kernels take as wmax, without
 *               a dasr_absmax pass; conv kernels only (transposed = 0), ldo <= DASR_AMAX_MAX_PARTS
 *   plain     : 1 = write the HWIO half only (two bias vectors side by side: O = n, I = KK = 1)
 *   wg_begin  : sum of the norm-group counts (O, or I when transposed) of the jobs before this one */
typedef struct dasr_pack_job {
    const float* v; const float* g; void* w; float* inv_norm; float* amax;
    int O, I, KK, transposed, ldo, o_off, bf16, plain, wg_begin, reserved;
} dasr_pack_job;
int dasr_weight_pack_multi(const dasr_pack_job* jobs_host, const dasr_pack_job* jobs_device, int njobs, void* stream);
/* given dW (HWIO): dv (layout of v) and dg ([O or I]); g == NULL: dv = unpacked dW, dg untouched. */
int dasr_weight_pack_bwd(const float* dw_hwio, const float* v, const float* g, const float* inv_norm, float* dv,
                         float* dg, int O, int I, int KH, int KW, int transposed, int ldo, int o_off, void* stream);

/* ---- convolution (NHWC, HWIO) -------------------------------------------------------------
 * Replaces nn.Conv2d / nn.ConvTranspose2d (+ bias, + LeakyReLU/ReLU, + nn.PixelShuffle, + the
 * residual add of Classic_Residual_Block) at sftmd_arch.py:743-749,811-820,861-866,133-151,891-910
 * and normalization.py:37-42.
 *   transposed = 0:  y[b,oy,ox,co] = bias[co] + sum x[b, oy*stride-pad+kh, ox*stride-pad+kw, ci] * w[kh,kw,ci,co]
 *   transposed = 1:  ConvTranspose2d geometry, Ho = (H-1)*stride - 2*pad + KH.
 * Epilogue: (+ residual[b,oy,ox,co]) -> act -> PixelShuffle(ps_r):
 *   ps_r > 1 writes y as [B][Ho*r][Wo*r][Cout/r^2] with
 *   y[b, oy*r+i, ox*r+j, c] = act(conv[b,oy,ox, c*r*r + i*r + j])   (bit-exact index map of nn.PixelShuffle).
 * bias, residual may be NULL.
 * y_amax (may be NULL): amax buffer (see dasr_absmax) for max |y|, filled by the mask layer's kernel while it stores and
 * by a pass over y after every other kernel.
 */
int dasr_conv2d_fwd(const float* x, const float* w_hwio, const float* bias, const float* residual, float* y, float* y_amax,
                    int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                    int transposed, int act, int ps_r, void* stream);
/* Read-only query for tests: the pixel-tile rows of the MFMA kernel that dasr_conv2d_fwd / dasr_conv2d_fwd_stats run for a
 * 3x3 / stride 1 / pad 1 convolution of this geometry - 8 (256-thread workgroups) or 16 (512-thread workgroups) - and 0
 * where another kernel family carries it.  The data gradient of a Cin -> Cout layer runs the form of (Cout, Cin). */
int dasr_conv2d_fwd_tile_rows(int B, int H, int W, int Cin, int Cout);
/* dasr_conv2d_fwd for a 3x3 / stride 1 / pad 1 convolution with bias and no activation, PLUS the statistics
 * nn.InstanceNorm2d(affine=False) needs of its output (sftmd_arch.py:811-820: `conv1 = Sequential(Conv2d, InstanceNorm2d)`):
 * mean[b,c], var[b,c] (biased) over the H*W pixels, as dasr_instnorm_stats(y) returns them.  On the MFMA path the
 * per-tile (mean, M2) pairs come out of the convolution's epilogue (no second pass over y) and are merged in tile
 * order with Chan's update; other shapes run the two entry points back to back.
 * workspace: dasr_conv2d_fwd_stats_workspace() bytes. */
size_t dasr_conv2d_fwd_stats_workspace(int B, int H, int W, int Cin, int Cout);
int dasr_conv2d_fwd_stats(const float* x, const float* w, const float* bias, float* y, float* mean, float* var,
                          void* workspace, size_t workspace_bytes, int B, int H, int W, int Cin, int Cout, void* stream);

/* Backward of the epilogue: dconv[b,oy,ox,cc] = dy[...shuffled...] * act'(y[...]) (y = saved forward output).
 * dconv_amax (may be NULL): amax buffer (see dasr_absmax) for max |dconv|, filled by the kernel. */
int dasr_conv2d_epilogue_bwd(const float* dy, const float* y, float* dconv, float* dconv_amax, int B, int Ho, int Wo,
                             int Cout, int act, int ps_r, void* stream);
/* dx (+)= conv-transpose of dconv with w; accumulate != 0 adds into dx. */
int dasr_conv2d_dgrad(const float* dconv, const float* w_hwio, float* dx, int accumulate, int B, int H, int W, int Cin,
                      int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int transposed, void* stream);
/* Data gradient fused with the PRODUCER's epilogue backward.  When the conv input x is the activated (and possibly
 * pixel-shuffled) output of another convolution - x = PixelShuffle_r(act(prev)) - and this conv is its only
 * consumer, the gradient w.r.t. prev is  dprev = unshuffle_r( dgrad(dconv) * act'(x) ):  the activation mask is
 * applied in the dgrad epilogue and the store goes through the inverse PixelShuffle index map, so the producer
 * needs no dasr_conv2d_epilogue_bwd pass.  x_act = this conv's saved input [B,H,W,Cin];
 * dprev [B, H/r, W/r, Cin*r*r].  dasr_conv2d_dgrad_act_supported() tells whether a kernel exists. */
int dasr_conv2d_dgrad_act_supported(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                    int pad, int transposed, int ps_r);
int dasr_conv2d_dgrad_act(const float* dconv, const float* w_hwio, const float* x_act, float* dprev, int B, int H, int W,
                          int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int transposed,
                          int act, int ps_r, void* stream);
/* dw_hwio = sum_pixels x (x) dconv ; dbias[co] = sum dconv (dbias may be NULL).
 * workspace: dasr_conv2d_wgrad_workspace() bytes. */
size_t dasr_conv2d_wgrad_workspace(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                   int pad, int transposed);
int dasr_conv2d_wgrad(const float* x, const float* dconv, float* dw_hwio, float* dbias, void* workspace,
                      size_t workspace_bytes, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                      int stride, int pad, int transposed, void* stream);

/* Weight/bias gradient with the activation backward fused in: dconv = dy * act'(y) is formed on the fly where a
 * fused kernel exists (Cin == 1: SEAN.mlp_mask; Cin == 3: the encoder's first layer) and is materialised into
 * dconv_scratch [B,Ho,Wo,Cout] otherwise (dconv_scratch may be NULL only where dasr_conv2d_wgrad_act_fused() returns 1).
 * For layers whose input needs no gradient. */
int dasr_conv2d_wgrad_act_fused(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                                int transposed);
int dasr_conv2d_wgrad_act(const float* x, const float* dy, const float* y, float* dw_hwio, float* dbias,
                          float* dconv_scratch, void* workspace, size_t workspace_bytes, int B, int H, int W, int Cin,
                          int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int transposed, int act,
                          void* stream);

/* ---- fp32 convolutions at fp32 accuracy on the BF16 matrix cores ("split bf16", csrc/conv_split_bf16.hip) ----------
 * For the plain (bias-only) 3x3 / stride 1 / pad 1 trunk convolutions of the fp32 path - mlp_gamma_o | mlp_beta_o
 * (normalization.py:41-42,73-74) and the DGB convolutions (sftmd_arch.py:811-820): every fp32 operand is the exact sum
 * of three bf16 pieces, six bf16 MFMAs per product term give the fp32 product to 2^-26, accumulated in fp32 - the
 * accuracy of the exact-fp32 MFMA kernels at 6/16 of their matrix time.  Replaces the same nn.Conv2d calls as
 * dasr_conv2d_fwd / dasr_conv2d_dgrad / dasr_conv2d_wgrad; Cin % 32 == 0, Cout % 32 == 0.
 *   split_weights: the fp32 packed kernel [2][3][3][Cin][Cout] -> a bf16 image (split_weights_bytes) holding, for the
 *                  forward and the dgrad, the three pieces of every K-step's slice contiguously (once per step)
 *   fwd_split:     y = act(conv(x, w) + bias + residual), optionally stored through PixelShuffle(2) (then no residual,
 *                  Cout % 128 == 0)                 x [B,H,W,Cin], y [B,H,W,Cout] fp32
 *   dgrad_split:   dx (+)= conv^T(dconv, w)         dconv [B,H,W,Cout], dx [B,H,W,Cin] fp32
 *   wgrad_split:   dw_hwio [3][3][Cin][Cout] = sum_pixels x (x) dconv, dbias (may be NULL) = sum dconv; workspace:
 *                  dasr_conv3x3_wgrad_split_workspace() bytes (replaces dasr_conv2d_wgrad for these layers) */
int dasr_conv3x3_split_supported(int H, int W, int Cin, int Cout);
size_t dasr_conv3x3_split_weights_bytes(int Cin, int Cout);
int dasr_conv3x3_split_weights(const float* w_packed, unsigned short* w_split, int Cin, int Cout, void* stream);
int dasr_conv3x3_fwd_split(const float* x, const unsigned short* w_split, const float* bias, const float* residual, float* y,
                           int B, int H, int W, int Cin, int Cout, int act, int ps_r, void* stream);
int dasr_conv3x3_dgrad_split(const float* dconv, const unsigned short* w_split, float* dx, int accumulate, int B, int H,
                             int W, int Cin, int Cout, void* stream);
size_t dasr_conv3x3_wgrad_split_workspace(int B, int H, int W, int Cin, int Cout);
int dasr_conv3x3_wgrad_split(const float* x, const float* dconv, float* dw_hwio, float* dbias, void* workspace,
                             size_t workspace_bytes, int B, int H, int W, int Cin, int Cout, void* stream);

/* The same convolutions with TWO fp16 pieces per operand and THREE products per term ("split fp16 x 2", same source file):
 * fp16 holds 11 significant bits, a pair 22-23 of fp32's 24 (0.5 ulp RMS off - one more fp32 rounding per operand), the
 * dropped term is 2^-24 relative, and only half as many partial sums are rounded into the fp32 accumulator: measured
 * against float64 the result is closer than both the bf16 x 3 scheme and the exact-fp32 MFMA kernels.  fp16's narrow range
 * is handled by a power-of-two scale per tensor that puts its largest magnitude in [2^14, 2^15):
 *   dasr_absmax:     max |x| over n floats (x 16-byte aligned) into an AMAX BUFFER: DASR_AMAX_FLOATS floats of device
 *                    memory, word 0 = the number n of partial maxima that follow (int), words 1 .. n = one partial maximum
 *                    per workgroup of the producing launch.  No atomics, nothing to clear, nothing read back by the host:
 *                    the kernels below take the maximum of the parts in their prologue and derive the scale from its
 *                    exponent bits.  Every `*max` / `*_amax` argument of this header is such a buffer; the producer-side
 *                    ones (y_amax, out_amax, dt_amax, ...) may be NULL and are filled by the kernel that writes the
 *                    tensor - no extra pass over it - or, where that kernel does not keep a maximum, by a follow-up pass
 *                    inside the entry point
 *   split2_weights:  wmax = dasr_absmax of the packed kernel's plane 0 (9 Cin Cout floats); image: split2_weights_bytes
 *   fwd / dgrad / wgrad_split2: as the functions above plus the maxima of their tensor operands (xmax of x, dmax of dconv);
 *                    y_amax (may be NULL): amax buffer for max |y| of what the forward stores, for the NEXT split convolution
 * Same nn.Conv2d calls replaced (normalization.py:41-42,73-74; sftmd_arch.py:811-820 and the upscale tail :891-909). */
#define DASR_AMAX_MAX_PARTS 4096
#define DASR_AMAX_FLOATS (1 + DASR_AMAX_MAX_PARTS)
int dasr_absmax(const float* x, size_t n, float* amax, void* stream);
size_t dasr_conv3x3_split2_weights_bytes(int Cin, int Cout);
int dasr_conv3x3_split2_weights(const float* w_packed, const float* wmax, unsigned short* w_split, int Cin, int Cout,
                                void* stream);
/* ... of every split convolution of a network in one launch (as dasr_weight_pack_multi: host and device copy of the job table;
 * wg_begin = sum of dasr_conv3x3_split2_weights_slabs(Cin, Cout) of the jobs before) */
typedef struct dasr_split_job {
    const float* w_packed; const float* wmax; unsigned short* w_split;
    int Cin, Cout, wg_begin, reserved;
} dasr_split_job;
int dasr_conv3x3_split2_weights_slabs(int Cin, int Cout);
int dasr_conv3x3_split2_weights_multi(const dasr_split_job* jobs_host, const dasr_split_job* jobs_device, int njobs, void* stream);
int dasr_conv3x3_fwd_split2(const float* x, const float* xmax, const unsigned short* w_split, const float* wmax,
                            const float* bias, const float* residual, float* y, float* y_amax, int B, int H, int W, int Cin,
                            int Cout, int act, int ps_r, void* stream);
int dasr_conv3x3_dgrad_split2(const float* dconv, const float* dmax, const unsigned short* w_split, const float* wmax,
                              float* dx, int accumulate, int B, int H, int W, int Cin, int Cout, void* stream);
int dasr_conv3x3_wgrad_split2(const float* x, const float* xmax, const float* dconv, const float* dmax, float* dw_hwio,
                              float* dbias, void* workspace, size_t workspace_bytes, int B, int H, int W, int Cin, int Cout,
                              void* stream);
/* dasr_conv3x3_dgrad_split2 with the PRODUCER's epilogue backward in its own epilogue, for Cin == 32 (the kernel that produces
 * 32 channels: the HR tail).  x_act [B,H,W,Cin] = this convolution's saved input = the producer's output behind its
 * activation `act` (none / ReLU / LeakyReLU(0.2)) and, with ps_r == 2, its PixelShuffle(2).
 *   ps_r == 1: dprev [B,H,W,Cin] = (dx (+ the old dprev if accumulate)) * act'(x_act) - the derivative applies to the SUM
 *   ps_r == 2: dprev [B,H/2,W/2,4 Cin], dprev[..][4c + 2(y&1) + (x&1)] = dx[y][x][c] * act'(x_act[y][x][c]); H, W even, no accumulate
 * Bit for bit what dasr_conv2d_epilogue_bwd makes of dasr_conv3x3_dgrad_split2's result, without the pass over it.
 * dprev_amax (may be NULL): amax buffer for max |dprev|.  DASR_E_UNSUPPORTED where dasr_conv3x3_dgrad_act_supported() is 0. */
int dasr_conv3x3_dgrad_act_supported(int H, int W, int Cin, int Cout, int act, int ps_r, int accumulate);
int dasr_conv3x3_dgrad_act_split2(const float* dconv, const float* dmax, const unsigned short* w_split, const float* wmax,
                                  const float* x_act, float* dprev, float* dprev_amax, int accumulate, int B, int H, int W,
                                  int Cin, int Cout, int act, int ps_r, void* stream);

/* The 9x9 output convolution (conv_output, sftmd_arch.py:910,948: Cin % 32 == 0 -> Cout <= 3, pad 4) in the same fp16 x 2
 * scheme (csrc/conv9_split.hip): fp32 x / w / y / dy / dx / dw, operands split into two scaled fp16 pieces when they are
 * staged.  w_hwio = the packed kernel's plane 0 [9][9][Cin][Cout]; xmax / dmax / wmax: amax buffers (dasr_absmax) of x,
 * dconv and w_hwio.  Replaces dasr_conv2d_fwd / _dgrad / _wgrad for that layer (same results to fp32 accuracy). */
int dasr_conv9_split_supported(int H, int W, int Cin, int Cout);
int dasr_conv9_fwd_split2(const float* x, const float* xmax, const float* w_hwio, const float* wmax, const float* bias, float* y,
                          int B, int H, int W, int Cin, int Cout, void* stream);
int dasr_conv9_dgrad_split2(const float* dconv, const float* dmax, const float* w_hwio, const float* wmax, float* dx,
                            int accumulate, int B, int H, int W, int Cin, int Cout, void* stream);
/* dasr_conv9_dgrad_split2 with the producer's epilogue backward in its own epilogue (what dasr_conv2d_dgrad_act is to
 * dasr_conv2d_dgrad): x_act = this convolution's saved input [B,H,W,Cin] = PixelShuffle(2)(act(prev conv)), its only consumer;
 * dprev [B, H/2, W/2, 4 Cin], dprev[..][4c + 2(y&1) + (x&1)] = dx[y][x][c] * act'(x_act[y][x][c]) - bit for bit what
 * dasr_conv2d_epilogue_bwd makes of dasr_conv9_dgrad_split2's dx, without dx ever reaching memory.  amax (may be NULL): amax
 * buffer for max |dprev|.  DASR_E_UNSUPPORTED unless ps_r == 2, H and W are even, act is none / ReLU / LeakyReLU(0.2) and
 * dasr_conv9_split_supported(H, W, Cin, Cout). */
int dasr_conv9_dgrad_act_split2(const float* dconv, const float* dmax, const float* w_hwio, const float* wmax, const float* x_act,
                                float* dprev, float* amax, int B, int H, int W, int Cin, int Cout, int act, int ps_r,
                                void* stream);
size_t dasr_conv9_wgrad_split2_workspace(int B, int H, int W, int Cin, int Cout);
int dasr_conv9_wgrad_split2(const float* x, const float* xmax, const float* dconv, const float* dmax, float* dw_hwio, float* dbias,
                            void* workspace, size_t workspace_bytes, int B, int H, int W, int Cin, int Cout, void* stream);

/* ---- instance-norm statistics ---------------------------------------------------------------
 * nn.InstanceNorm2d(affine=False) appears twice in a row on every DGB conv output
 * (sftmd_arch.py:811-820 then normalization.py:16-17,56).  Both collapse to one per-(b,c) scale:
 *   xhat = (x - mean) * rsqrt(var+eps) * rsqrt(var/(var+eps) + eps)      
 * This entry point computes mean and biased variance per (b,c) of an NHWC tensor
 * (chunked two-pass + Chan merge in a fixed order: no E[x^2]-mean^2 cancellation, bitwise reproducible).
 * workspace: dasr_instnorm_stats_workspace() bytes.
 */
size_t dasr_instnorm_stats_workspace(int B, int HW, int C);
int dasr_instnorm_stats(const float* x, float* mean, float* var, void* workspace, size_t workspace_bytes, int B, int HW,
                        int C, void* stream);

/* ---- depth matrix -> per-sample dynamic kernels ------------------------------------------------
 * SEAN.A_i_j (1x1 conv over the K axis) and the collapse of mlp_gamma_s / mlp_beta_s over the
 * style map (normalization.py:27-29,80-85):
 *   stp[b,k,l]       = A_b[k] + sum_j A_w[k,j] * st[b,j,l]
 *   D[b,s,tap,k,c]   = sum_l W_s[c,l,tap] * stp[b,k,l]          s = 0 (gamma), 1 (beta); tap = kh*3+kw
 * W_gamma / W_beta are the module's OIHW tensors [C][L][3][3].  Any L > 0, odd ones included, forward and backward.
 */
int dasr_dynk_fwd(const float* st, const float* A_w, const float* A_b, const float* W_gamma, const float* W_beta,
                  float* stp, float* D, int B, int K, int L, int C, void* stream);
/* Given dD: dW_gamma, dW_beta (written), dA_w, dA_b (written), dst (ACCUMULATED: the depth matrix feeds every SEAN).
 * dstp is a [B,K,L] scratch. */
int dasr_dynk_bwd(const float* dD, const float* st, const float* stp, const float* A_w, const float* W_gamma,
                  const float* W_beta, float* dW_gamma, float* dW_beta, float* dA_w, float* dA_b, float* dst,
                  float* dstp, int B, int K, int L, int C, void* stream);

/* ---- the Depth-Guided Block's dynamic convolution + DFN modulation (north-star kernel) ----------
 * Replaces, per SEAN call (normalization.py:56,59,80-89) and the surrounding ReLU / residual of
 * Depth_Residual_Block_Mask.forward (sftmd_arch.py:826-834):
 *   xhat   = double instance norm of t (stats from dasr_instnorm_stats)
 *   gamma1 = bias_gamma[c] + sum_{tap,k} mask[b,k,p+tap] * D[b,0,tap,k,c]       (zero padding)
 *   beta1  = bias_beta[c]  + sum_{tap,k} mask[b,k,p+tap] * D[b,1,tap,k,c]
 *   gamma  = a_g*gamma1 + (1-a_g)*gamma2 ;  beta = a_b*beta1 + (1-a_b)*beta2
 *   out    = xhat*(1+gamma) + beta  (+ residual)  -> ReLU if relu != 0
 * t, out, residual: NHWC [B,H,W,C]; gb2: NHWC [B,H,W,2C] (gamma2 | beta2 = mlp_gamma_o | mlp_beta_o outputs);
 * mask: NCHW [B,K,H,W] as the reference delivers it (any float values); bias_gamma/bias_beta [C] are the
 * mlp_gamma_s / mlp_beta_s biases; alpha_gamma / alpha_beta are 1-element DEVICE tensors (trainable, normalization.py:30-35).
 * region / onehot_flag: outputs of dasr_mask_compress for the same mask.  Both NULL: general kernel only.
 * The general (soft-mask) kernels run the dynamic convolution as a per-sample GEMM on the exact-fp32 matrix cores
 * (contraction over the 9*K (tap, region) pairs; backward: dD = A^T . [dgamma1 | dbeta1] over the pixels, per-workgroup
 * slabs summed in a fixed order) when C % 4 == 0, for K up to 16; C % 4 != 0 falls back to scalar kernels, K <= 14.
 * Both given: both kernels are launched and the flag decides ON THE DEVICE which one works.  region given and
 * onehot_flag NULL: the caller has read the flag (== 0) itself and vouches for one-hot masks: gather kernel only.
 */
/* One byte per pixel from the K mask planes: region[b,y,x] = k if mask[b,k,y,x] == 1 and every other plane is 0,
 * K if all planes are 0; *onehot_flag is set to a non-zero value if ANY pixel is neither (soft / overlapping
 * masks).  The SEAN entry points run a gather kernel when the flag is 0 and the general kernel otherwise; the
 * choice is made on the device, the host never reads the flag.  A pixel that no plane claims (byte K) adds nothing
 * to gamma1 / beta1: where a whole 3x3 neighbourhood is unclaimed they are the bare biases, forward and backward. */
int dasr_mask_compress(const float* mask, unsigned char* region, int* onehot_flag, int B, int K, int H, int W,
                       void* stream);
int dasr_sean_fwd(const float* t, const float* mean, const float* var, const float* gb2, const float* mask,
                  const unsigned char* region, const int* onehot_flag, const float* D, const float* bias_gamma, const float* bias_beta, const float* alpha_gamma,
                  const float* alpha_beta, const float* residual, float* out, float* out_amax, int relu, int B, int H,
                  int W, int C, int K, float eps, void* stream);
/* Backward. Inputs as forward plus dout and the saved forward output `out` (for the ReLU mask).
 * Outputs: dt [B,H,W,C]; dgb2 [B,H,W,2C]; dD [B,2,9,K,C]; dbias_gamma, dbias_beta [C]; dalpha_gamma, dalpha_beta [1];
 * dres (may be NULL; written = dout*relu') ; workspace: dasr_sean_bwd_workspace() bytes.
 * out_amax / dt_amax / dgb2_amax (fp32 entry points, each may be NULL): amax buffers (see dasr_absmax) that receive
 * max |.| of the tensor just written, for the fp16 x 2 split convolution that reads it next. */
size_t dasr_sean_bwd_workspace(int B, int H, int W, int C, int K);
int dasr_sean_bwd(const float* dout, const float* out, const float* t, const float* mean, const float* var,
                  const float* gb2, const float* mask, const unsigned char* region, const int* onehot_flag,
                  const float* D, const float* bias_gamma, const float* bias_beta,
                  const float* alpha_gamma, const float* alpha_beta, float* dt, float* dgb2, float* dD,
                  float* dbias_gamma, float* dbias_beta, float* dalpha_gamma, float* dalpha_beta, float* dres,
                  float* dt_amax, float* dgb2_amax, void* workspace, size_t workspace_bytes, int relu, int B, int H, int W,
                  int C, int K, float eps, void* stream);

/* Largest K for which the soft-mask (general) kernels run forward and backward: 16, the same as for one-hot masks
 * (C % 4 == 0; the scalar fallback for other channel counts returns DASR_E_UNSUPPORTED above K = 14). */
int dasr_sean_soft_mask_max_regions(void);

/* ---- region-wise average pooling (depth matrix) ---------------------------------------------------
 * RegionWiseAvgPooling.forward (sftmd_arch.py:714-733): masks are resized to the feature size with
 * bilinear(align_corners=True) and re-binarised (>= 0.5) when sizes differ; per region
 *   out[b,k,l] = sum_p m[b,k,p]*feat[b,p,l] / (sum_p m[b,k,p] + 1e-10).
 * feat NHWC [B,h,w,L]; mask NCHW [B,K,H,W]; maskr NCHW [B,K,h,w] and area [B,K] are written and
 * kept for the backward.
 */
int dasr_region_pool_fwd(const float* feat, const float* mask, float* maskr, float* area, float* out, int B, int K,
                         int L, int h, int w, int H, int W, void* stream);
int dasr_region_pool_bwd(const float* dout, const float* maskr, const float* area, float* dfeat, int B, int K, int L,
                         int h, int w, void* stream);

/* ---- device-side input preparation ------------------------------------------------------
 * Replaces LQGTker_Depth_dataset.getDepthMask (codes/data/LQGTker_Depth_dataset.py:204-225) + the host-side
 * stacking of the K float planes (:155-158,196): per sample, K equal-width half-open bins over the map's own
 * [min, max] (float32 arithmetic as torch evaluates it: interval = (max-min)/K, edge_i = min + interval*i); a
 * pixel equal to the maximum belongs to no bin.  depth: [B,HW] float32.  Outputs (either may be NULL, not both):
 * masks NCHW [B,K,HW] of 0/1 floats (what DepthNet.forward takes) and region bytes [B,HW] (k, or K for "no bin":
 * what the one-hot SEAN / loss kernels read - identical to dasr_mask_compress of those planes).
 * fixed_edges: NULL for the data-dependent range (depthFixedRange: false, every shipped yml); else K+1 DEVICE
 * floats holding the edges of the fixed [0,1] range (the reference computes those in Python doubles; the host
 * wrapper passes them rounded to float32, which is what torch compares against).
 * workspace: dasr_depth_to_masks_workspace() bytes (per-chunk minima / maxima). */
size_t dasr_depth_to_masks_workspace(int B, int HW);
int dasr_depth_to_masks(const float* depth, const float* fixed_edges, float* masks, unsigned char* region,
                        void* workspace, size_t workspace_bytes, int B, int HW, int K, void* stream);

/* dasr_depth_to_masks_soft: soft (hat-function) membership in the same K bins, for the soft-mask kernels.  Per sample
 * lo, hi = min, max of the map (fixed_range != 0: lo = 0, hi = 1 and no min / max pass), interval = (hi - lo) / K, and
 * per pixel, in float32 with every operation rounded on its own (no FMA contraction, IEEE division):
 *   interval not > 0 (constant map): plane 0 = 1, all others 0 (the one-hot rule leaves such a map in no bin)
 *   u = min(max((v - lo) / interval, 0), K)         fixed range: values outside [0,1] go to the end planes
 *   k = min((int)floorf(u), K - 1);  r = u - k      r in [0,1]; r == 1 only at u == K, the maximum
 *   r < 0.5:  n = k - 1, s = 0.5 - r / width        else:  n = k + 1, s = 0.5 - (1 - r) / width
 *   s = max(s, 0), and s = 0 where n < 0 or n >= K;  plane[k] = 1 - s, plane[n] = s, every other plane 0
 * width = 1: linear interpolation between bin centres; a smaller width narrows the blend to a band of width * interval
 * around each interior edge (0.5 / 0.5 on the edge, from both sides); width -> 0 tends to the binning above.  At most two
 * planes are non-zero per pixel and they sum to 1; every plane is Lipschitz in v with constant 1 / (interval * width).
 * The MAXIMUM pixel belongs to plane K-1 here; the one-hot rule above (the reference's) leaves it in no bin.
 * NaN depth: unspecified.  masks: NCHW [B,K,HW] float32, every element written (no memset needed); any alignment (16-byte
 * stores where the address allows, scalar stores elsewhere).  0 < width <= 1, else (NaN included) DASR_E_SHAPE;
 * K > 16: DASR_E_UNSUPPORTED.  workspace: dasr_depth_to_masks_soft_workspace() bytes (required in both modes). */
size_t dasr_depth_to_masks_soft_workspace(int B, int HW);
int dasr_depth_to_masks_soft(const float* depth, float* masks, void* workspace, size_t workspace_bytes, int B, int HW,
                             int K, float width, int fixed_range, void* stream);

/* ---- the pair encoding of a soft mask made by the rule above ------------------------------------------------------
 * At most two planes of such a mask are non-zero per pixel and the two are neighbours, so a pixel is described by two
 * side-cars next to the K planes:
 *   pair_k  uint8   [B,HW]  the plane k that holds 1 - s (the k of the rule); byte K = "no plane"
 *   pair_s  float32 [B,HW]  |pair_s| = s in [0, 0.5]; negative: the neighbour is n = k - 1, otherwise n = k + 1.
 *                           A pixel without a second plane (a bin centre, an end plane facing outwards, a constant
 *                           map) has s == 0, stored as +0.0 and never -0.0.
 * Decoding (THE rule, dasr_amd.prep.pair_planes restates it):
 *   plane[k] = fl32(1 - |pair_s|)  (the producer's own rounding of 1 - s),  plane[n] = |pair_s|,  every other plane 0;
 *   a k >= K, or an n outside 0..K-1, contributes nothing for that term - it is never used as an address.
 * These bytes are NOT the one-hot region bytes of dasr_mask_compress / dasr_depth_to_masks: they go to
 * dasr_sean_fwd_pair[_bf16] only, never to dasr_sean_bwd, the loss kernels or any `region` argument.
 *
 * dasr_depth_to_masks_soft_pair: dasr_depth_to_masks_soft with the two side-cars written by the same launch.  masks may
 * be NULL (the planes are then not written); pair_k and pair_s are required (DASR_E_NULL).  The planes are bit-identical
 * to dasr_depth_to_masks_soft's; refusals and workspace (dasr_depth_to_masks_soft_workspace) are the same. */
int dasr_depth_to_masks_soft_pair(const float* depth, float* masks, unsigned char* pair_k, float* pair_s, void* workspace,
                                  size_t workspace_bytes, int B, int HW, int K, float width, int fixed_range, void* stream);

/* dasr_sean_fwd for a mask in the pair encoding: the arguments of dasr_sean_fwd with (mask, region, onehot_flag)
 * replaced by (pair_k, pair_s) [B,H,W].  Computes what dasr_sean_fwd computes on the decoded planes, in the general
 * kernel's order of summation (taps 0..8, the two planes of a tap in ascending plane index, the bias after the chain),
 * with two row gathers per tap instead of the 9K-term contraction.  Forward only: the backward is dasr_sean_bwd on the
 * planes with region = onehot_flag = NULL.  C % 4 != 0 or K > 16: DASR_E_UNSUPPORTED before any launch.
 * out_amax (fp32 entry point, may be NULL): as in dasr_sean_fwd, kept by the kernel itself. */
int dasr_sean_fwd_pair(const float* t, const float* mean, const float* var, const float* gb2, const unsigned char* pair_k,
                       const float* pair_s, const float* D, const float* bias_gamma, const float* bias_beta,
                       const float* alpha_gamma, const float* alpha_beta, const float* residual, float* out,
                       float* out_amax, int relu, int B, int H, int W, int C, int K, float eps, void* stream);
int dasr_sean_fwd_pair_bf16(const unsigned short* t, const float* mean, const float* var, const unsigned short* gb2,
                            const unsigned char* pair_k, const float* pair_s, const float* D, const float* bias_gamma,
                            const float* bias_beta, const float* alpha_gamma, const float* alpha_beta,
                            const unsigned short* residual, unsigned short* out, int relu, int B, int H, int W, int C,
                            int K, float eps, void* stream);

/* ---- harness losses in one pass (one-hot and soft masks) ----------------------------------
 * nn.L1Loss + dynamic_weight_mask_loss('smoothl1') (F_model_depthCond.py:164,188-190; mask_loss.py:64-90) need, per
 * depth region k, sum smooth_l1(m_k*sr, m_k*hr) and sum m_k (masks nearest-upsampled to HR), and sum |sr-hr|.
 * sr, hr: NCHW [B,C,h*scale,w*scale]; region: bytes [B,h,w] from dasr_mask_compress.
 * sums [2K+1] = K numerators | K areas (C * #pixels) | sum|sr-hr|.  Division / softmax weights stay in PyTorch.
 * dasr_loss_bwd: dsr = dsums[2K]*sign(sr-hr) + dsums[region]*smooth_l1'(sr-hr)  (dsums: device [2K+1]). */
int dasr_loss_sums(const float* sr, const float* hr, const unsigned char* region, float* sums, int B, int C, int h,
                   int w, int scale, int K, void* stream);
int dasr_loss_bwd(const float* sr, const float* hr, const unsigned char* region, const float* dsums, float* dsr, int B,
                  int C, int h, int w, int scale, int K, void* stream);
/* The same sums for arbitrary float masks (negative values, zeros, values above 1; not one-hot): replaces the K masked
 * passes of dynamic_weight_mask_loss('smoothl1') (mask_loss.py:64-90) and nn.L1Loss (F_model_depthCond.py:164,188-190).
 * mask: NCHW [B,K,h,w] float32, nearest-upsampled by `scale` to M_k; d = sr - hr.
 * sums [2K+1], the layout of dasr_loss_sums: num_k = sum smooth_l1(M_k * d) (beta 1; the mask is INSIDE the
 * smooth-L1) | area_k = C * scale^2 * sum m_k | sum |d|.  K <= 16, else DASR_E_UNSUPPORTED.
 * dasr_loss_bwd_soft: dsr = dsums[2K]*sign(d) + sum_k dsums[k] * M_k * smooth_l1'(M_k * d); dsums[K..2K-1] is not read
 * (the harness detaches the areas) and the masks receive no gradient. */
int dasr_loss_sums_soft(const float* sr, const float* hr, const float* mask, float* sums, int B, int C, int h, int w,
                        int scale, int K, void* stream);
int dasr_loss_bwd_soft(const float* sr, const float* hr, const float* mask, const float* dsums, float* dsr, int B, int C,
                       int h, int w, int scale, int K, void* stream);
/* The same two passes with the criteria as ARGUMENTS - what a reference yml can switch on beside the defaults:
 * pixel_crit: train.pixel_criterion l1 | l2 | cb (nn.L1Loss / nn.MSELoss / CharbonnierLoss, F_model_depthCond.py:50-58,164;
 * loss.py:37-47); crit_a: dynamic_loss.dynamic_criterion l1 | l2 | smoothl1 (mask_loss.py:44-90); crit_b: a second region
 * criterion for mask_loss (mask_loss.py:6-41, F_model_depthCond.py:183-186) when mask_criterion differs from
 * dynamic_criterion, else DASR_CRIT_NONE.  They replace nn.L1Loss / nn.MSELoss / CharbonnierLoss on (sr, hr) and the K
 * (2K) masked passes of those two modules.  With d = sr - hr and M_k the nearest-upsampled mask:
 * sums = K numerators of A | K areas (as above) | pixel sum | with crit_b: K numerators of B   ([2K+1], [3K+1] with crit_b)
 *   pixel sum: sum |d| (l1), sum d^2 (l2), sum sqrt(d^2 + 1e-6) (cb)
 *   numerator k: sum |M_k d| (l1), sum (M_k d)^2 (l2), sum smooth_l1(M_k d), beta 1 (smoothl1); the mask is INSIDE
 * (region bytes: the criterion of d over the region's pixels).  Means / ratios / weights stay in PyTorch.
 * bwd: dsr = dsums[2K] * pix'(d) + sum_k M_k (dsums[k] A'(M_k d) + dsums[2K+1+k] B'(M_k d)), with l1' = sign (sign(0) = 0),
 * l2' = 2u, cb' = d / sqrt(d^2 + 1e-6), smooth_l1' = u for |u| < 1 else sign(u).  dsums: DEVICE vector of the sums' length
 * (the areas' entries are not read); nothing is read back to the host, so both passes can be captured.
 * cb as a region criterion, smoothl1 as the pixel criterion, any other code and K > 16: DASR_E_UNSUPPORTED before a launch.
 * (pixel l1, A smoothl1, no B) computes what the four entry points above compute; they remain what the defaults run. */
#define DASR_CRIT_NONE (-1)
#define DASR_CRIT_L1 0
#define DASR_CRIT_L2 1
#define DASR_CRIT_CB 2
#define DASR_CRIT_SMOOTHL1 3
int dasr_loss_sums_crit(const float* sr, const float* hr, const unsigned char* region, float* sums, int B, int C, int h,
                        int w, int scale, int K, int pixel_crit, int crit_a, int crit_b, void* stream);
int dasr_loss_bwd_crit(const float* sr, const float* hr, const unsigned char* region, const float* dsums, float* dsr,
                       int B, int C, int h, int w, int scale, int K, int pixel_crit, int crit_a, int crit_b, void* stream);
int dasr_loss_sums_soft_crit(const float* sr, const float* hr, const float* mask, float* sums, int B, int C, int h, int w,
                             int scale, int K, int pixel_crit, int crit_a, int crit_b, void* stream);
int dasr_loss_bwd_soft_crit(const float* sr, const float* hr, const float* mask, const float* dsums, float* dsr, int B,
                            int C, int h, int w, int scale, int K, int pixel_crit, int crit_a, int crit_b, void* stream);

/* ---- small elementwise helpers ---------------------------------------------------------------- */
int dasr_add(const float* a, const float* b, float* out, size_t n, void* stream);  /* torch.add, sftmd_arch.py:931 */
int dasr_accumulate(float* dst, const float* src, size_t n, void* stream);         /* dst += src (gradient fan-in) */
int dasr_copy(float* dst, const float* src, size_t n, void* stream);               /* device-to-device copy */

/* ==== mixed precision: bf16 activations (BASELINE.json configs[2..3]) ================================================
 * Replaces the same torch ops as the fp32 entry points when the reference is run under torch.autocast(bfloat16):
 * nn.Conv2d / weight_norm convs (sftmd_arch.py:811-820,891-910), SEAN (normalization.py:37-42,52-92).  Activation tensors
 * (unsigned short* = bf16 bits, NHWC) are bf16 in HBM; parameters, their gradients, instance-norm statistics, the dynamic
 * kernels D and every accumulator are fp32.  Same conventions as above (asynchronous, no allocation, return codes).
 * The bf16 path has no generic fallback kernels: unsupported geometries return DASR_E_UNSUPPORTED. */

/* dasr_weight_pack_fwd with a bf16 packed kernel (normalisation in fp32, one rounding); dasr_weight_pack_bwd serves both. */
int dasr_weight_pack_fwd_bf16(const float* v, const float* g, unsigned short* w, float* inv_norm, int O, int I, int KH, int KW,
                              int transposed, int ldo, int o_off, void* stream);
/* Convolution forward.  Three layer kinds, told apart by the geometry:
 *   trunk   3x3 / stride 1 / pad 1, Cin % 32 == 0, Cout % 32 == 0 : x bf16, w packed bf16, y / residual bf16
 *           (v_mfma_f32_32x32x16_bf16, fused bias / activation / PixelShuffle / residual as dasr_conv2d_fwd)
 *   mask    3x3, Cin == 1 (SEAN.mlp_mask on the depth map)         : x f32,  w packed f32,  y bf16
 *   output  9x9 / pad 4, Cout <= 3 (conv_output)                   : x bf16, w packed f32,  y f32 */
int dasr_conv2d_fwd_bf16(const void* x, const void* w, const float* bias, const unsigned short* residual, void* y, int B,
                         int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int transposed,
                         int act, int ps_r, void* stream);
int dasr_conv2d_epilogue_bwd_bf16(const unsigned short* dy, const unsigned short* y, unsigned short* dconv, int B, int Ho,
                                  int Wo, int Cout, int act, int ps_r, void* stream);
/* Which kernel runs the trunk's forward / dgrad: 0 (default) = the persistent LDS-DMA kernel (csrc/conv_bf16_v2.hip) where
 * it applies (Cin % 32 == 0, Cout % 64 == 0, PixelShuffle 1 or 2), 1 = the first, register-staged kernel everywhere,
 * 2 = the persistent kernel with one workgroup per XCD (tests: long per-workgroup item lists on small shapes);
 * + 16 = force its 8-row / 4-wave form, + 32 = its 16-row / 8-wave form (default: by problem size);
 * + 64 = the fp16 x 2 split weight gradient on its first kernel (operands split per K-step; default: split at staging);
 * + 256 = the fp16 x 2 split forward / dgrad at 128 produced channels in its four-wave form (four tile rows per wave);
 * + 512 = ... at 64 produced channels with all nine kernel slices of a chunk per barrier; + 1024 = swap its two eight-wave
 * forms (128 produced channels: kernel-row K-steps instead of channel halves x kernel columns; 64: the reverse);
 * + 2048 = the bf16 dynamic-conv forward (dasr_sean_fwd_bf16) with 4 instead of 8 channels per lane;
 * + 4096 = the first form of the 9x9 split forward (+ 8192) with the linear instead of the XCD-blocked tile order;
 * + 8192 = the 9x9 split forward in its first form (one 512-thread workgroup per CU on 8 x 56 tiles; default at Cin = 32: two
 * 256-thread workgroups per CU on 8 x 24 tiles in linear order, the same bits).
 * For A/B measurements and tests; process-wide, not thread-safe against concurrent launches.
 * dasr_conv_bf16_v2_launches(): how many times the persistent kernel has been launched by this process. */
int dasr_set_conv_bf16_impl(int impl);
int dasr_get_conv_bf16_impl(void);
int dasr_conv_bf16_v2_launches(void);
/* trunk: dconv bf16, w packed bf16; output conv: dconv f32, w packed f32.  dx bf16. */
int dasr_conv2d_dgrad_bf16(const void* dconv, const void* w, unsigned short* dx, int accumulate, int B, int H, int W, int Cin,
                           int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad, int transposed, void* stream);
size_t dasr_conv2d_wgrad_workspace_bf16(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                        int pad, int transposed);
/* trunk: x bf16, dconv bf16; output conv: x bf16, dconv f32.  dw (plain HWIO) and dbias fp32. */
int dasr_conv2d_wgrad_bf16(const unsigned short* x, const void* dconv, float* dw, float* dbias, void* workspace,
                           size_t workspace_bytes, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW,
                           int stride, int pad, int transposed, void* stream);
/* mask layer: weight / bias gradient with the activation backward fused (x = depth map f32, dy / y bf16). */
int dasr_conv2d_wgrad_act_bf16(const float* x, const unsigned short* dy, const unsigned short* y, float* dw, float* dbias,
                               int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad,
                               int transposed, int act, void* stream);
/* dasr_instnorm_stats / dasr_sean_fwd / dasr_sean_bwd on bf16 activations (t, gb2, residual, out and their gradients);
 * workspaces as for the fp32 entry points. */
int dasr_instnorm_stats_bf16(const unsigned short* x, float* mean, float* var, void* workspace, size_t workspace_bytes, int B,
                             int HW, int C, void* stream);
int dasr_sean_fwd_bf16(const unsigned short* t, const float* mean, const float* var, const unsigned short* gb2,
                       const float* mask, const unsigned char* region, const int* onehot_flag, const float* D,
                       const float* bias_gamma, const float* bias_beta, const float* alpha_gamma, const float* alpha_beta,
                       const unsigned short* residual, unsigned short* out, int relu, int B, int H, int W, int C, int K,
                       float eps, void* stream);
int dasr_sean_bwd_bf16(const unsigned short* dout, const unsigned short* out, const unsigned short* t, const float* mean,
                       const float* var, const unsigned short* gb2, const float* mask, const unsigned char* region,
                       const int* onehot_flag, const float* D, const float* bias_gamma, const float* bias_beta,
                       const float* alpha_gamma, const float* alpha_beta, unsigned short* dt, unsigned short* dgb2, float* dD,
                       float* dbias_gamma, float* dbias_beta, float* dalpha_gamma, float* dalpha_beta, unsigned short* dres,
                       void* workspace, size_t workspace_bytes, int relu, int B, int H, int W, int C, int K, float eps,
                       void* stream);
/* elementwise helpers (n % 4 == 0) and the casts at the fp32 encoder <-> bf16 trunk boundary */
int dasr_add_bf16(const unsigned short* a, const unsigned short* b, unsigned short* out, size_t n, void* stream);
int dasr_accumulate_bf16(unsigned short* dst, const unsigned short* src, size_t n, void* stream);
int dasr_cast_f32_to_bf16(const float* src, unsigned short* dst, size_t n, void* stream);
int dasr_cast_bf16_to_f32(const unsigned short* src, float* dst, int accumulate, size_t n, void* stream);

/* ---- the encoder's stride-2 layers on the bf16 stride-1 kernels (csrc/s2d.hip) -----------------------------------
 * Encoder (sftmd_arch.py:745-749, 771-783): nn.Conv2d(.., 3, stride=2, padding=1) x3 and
 * nn.ConvTranspose2d(.., 3, stride=2, padding=1) (no output_padding: (2H-1) x (2W-1) outputs).  With bf16 activations
 * they are expressed as stride-1 3x3 convolutions (dasr_conv2d_*_bf16) of a space-to-depth image / with a PixelShuffle(2)
 * epilogue (a 2H x 2W image whose last row and column the reference's layer does not have):
 *   space_to_depth2:        y[b][i][j][(2py+px)C + c] = x[b][2i+py][2j+px][c] for 2i+py < Hv, 2j+px < Wv, zero beyond
 *                           the VALID extents (Hv <= H, Wv <= W: H, W for a plain tensor; 2H'-1, 2W'-1 for the
 *                           PixelShuffle image of the transposed layer); x fp32 or bf16
 *   depth_to_space2_bwd:    the adjoint (gradient of the above: zero beyond the valid extents), into an fp32 or bf16
 *                           tensor, optionally accumulating
 *   weight_expand_s2:       fp32 HWIO [3][3][Cin][Cout] -> the bf16 packed kernel [2][3][3][4Cin][Cout] of the stride-1 form
 *   weight_collapse_s2:     fp32 gradient of the expanded kernel [3][3][4Cin][Cout] -> [3][3][Cin][Cout]
 *   weight_expand_t2 / weight_collapse_t2: the same for the transposed convolution: [3][3][Cin][Cout] <-> Cin -> 4 Cout
 *                           (output channel 4co + 2a + b = phase (a, b) of the PixelShuffle), bias repeated / summed.
 * All C % 4 == 0. */
int dasr_space_to_depth2_bf16(const void* x, int x_is_bf16, unsigned short* y, int B, int H, int W, int C, int Hv, int Wv,
                              void* stream);
int dasr_depth_to_space2_bwd_bf16(const unsigned short* dy, void* dx, int dx_is_bf16, int accumulate, int B, int H, int W,
                                  int C, int Hv, int Wv, void* stream);
int dasr_weight_expand_s2_bf16(const float* w_hwio, unsigned short* out, int Cin, int Cout, void* stream);
int dasr_weight_collapse_s2(const float* dw_expanded, float* dw_hwio, int Cin, int Cout, void* stream);
int dasr_weight_expand_t2_bf16(const float* w_hwio, const float* bias, unsigned short* out, float* bias_out, int Cin,
                               int Cout, void* stream);
int dasr_weight_collapse_t2(const float* dw_expanded, const float* dbias_expanded, float* dw_hwio, float* dbias, int Cin,
                            int Cout, void* stream);

/* ---- SSIM (validation metric) -------------------------------------------------------------------------------------
 * pytorch_ssim.ssim (reference codes/pytorch_ssim/__init__.py:17-37,65-73; train.py:239): 11 x 11 Gaussian windows
 * (sigma 1.5, zero padding), C1 = 0.01^2, C2 = 0.03^2, images [B,C,H,W] fp32 in [0,1].  One pass over both images:
 * out_per_sample[b] = mean over (C,H,W) of the SSIM map (their mean over b is size_average=True).  window11: HOST
 * pointer to the eleven normalised 1-D window weights.  workspace: dasr_ssim_workspace() bytes. */
size_t dasr_ssim_workspace(int B, int C, int H, int W);
int dasr_ssim(const float* img1, const float* img2, const float* window11, float* out_per_sample, void* workspace,
              size_t workspace_bytes, int B, int C, int H, int W, void* stream);
/* The same quantity as a training criterion (models/modules/ssim_loss.py, F_model_depthCond.py:179): with
 * S = mean over (B,C,H,W) of the SSIM map, dimg1 (=|+=) dscale[0] * dS/dimg1, in one launch that reads img1, img2 and
 * writes dimg1 - nothing is saved by dasr_ssim for it (csrc/ssim_bwd.hip).  No gradient to img2.  dscale: DEVICE pointer to
 * one float (dL/dS), read by the kernel: no host read-back, the call can be captured.  accumulate != 0 adds into dimg1
 * (every element is written by exactly one thread), 0 overwrites.  window11: HOST pointer as above. */
int dasr_ssim_bwd(const float* img1, const float* img2, const float* window11, const float* dscale, float* dimg1,
                  int accumulate, int B, int C, int H, int W, void* stream);

/* ---- video frames: the uint8 edge of inference (csrc/frame.hip) ----------------------------------------------------
 * A camera frame is uint8 HWC (BGR as cv2 delivers it); the network is NHWC inside.  These three keep the host out of the
 * per-frame path: one byte per sample crosses PCIe in each direction and no layout pass runs on either side.
 *
 * dasr_frame_ingest_u8: frames uint8 [B,H,W,C] -> x_nhwc float [B,H,W,C] = frames / 255 (IEEE division, bit-identical
 * to `img.astype(np.float32) / 255.`); swap_rb != 0 with C == 3 reverses the channel order (BGR -> RGB).  Replaces
 * read_img's `astype(np.float32) / 255.` (codes/data/util.py:78) and img2tensor (codes/utils/util.py:596-605: the same
 * division, `[:, :, [2, 1, 0]]`, `transpose(2, 0, 1)`) together with dasr_nchw_to_nhwc. */
int dasr_frame_ingest_u8(const unsigned char* frames, float* x_nhwc, int B, int H, int W, int C, int swap_rb,
                         void* stream);
/* dasr_frame_emit_u8: y_nhwc float [B,H,W,C] (conv_output's result BEFORE the clamp) -> frames uint8 [B,H,W,C]:
 *   v = clamp(y, net_lo, net_hi)                         torch.clamp(out, min, max), sftmd_arch.py:950
 *   v = clamp(v, mm_lo, mm_hi); v = (v - mm_lo) / (mm_hi - mm_lo); u = rint(v * 255)      tensor2img, utils/util.py:572-590
 * in fp32, ties to even (numpy's round), bit-identical to tensor2img(dasr_clamp_to_nchw(y)[b], min_max=(mm_lo, mm_hi)) for
 * every finite y (NaN: unspecified).  mm_lo / mm_hi are doubles because tensor2img forms `max - min` in Python doubles
 * before torch rounds it to float32.  swap_rb != 0 with C == 3 writes BGR (tensor2img's `[[2, 1, 0], :, :]`).
 * C must be 1 or 3 (DASR_E_UNSUPPORTED otherwise); mm_hi > mm_lo.
 * Alignment (ingest and emit): any addresses are accepted, but the wide path (12 bytes / three 16-byte accesses per lane)
 * needs an element offset at which the uint8 address is a multiple of 4 AND the float address a multiple of 16; pass a
 * 4-byte-aligned uint8 buffer and a 16-byte-aligned float buffer (any hipMalloc result) to get it - with incompatible
 * residues the whole batch goes one element per lane, correct but several times slower. */
int dasr_frame_emit_u8(const float* y_nhwc, unsigned char* frames, int B, int H, int W, int C, float net_lo, float net_hi,
                       double mm_lo, double mm_hi, int swap_rb, void* stream);
/* dasr_frame_ssd_u8: ssd[b] = sum over rows / columns crop .. H-1-crop / W-1-crop and all C channels of (a - b)^2, exact
 * (unsigned 64-bit), for two uint8 [B,H,W,C] image batches: the `mse` of calculate_psnr (utils/util.py:646-653) times the
 * sample count, on the cropped uint8 images codes/train.py:245-262 hands it.  PSNR = 20 log10(255 / sqrt(ssd / n)),
 * n = (H - 2 crop)(W - 2 crop) C.  2 crop >= H or 2 crop >= W: DASR_E_UNSUPPORTED.
 * workspace: dasr_frame_ssd_u8_workspace() bytes (one 64-bit partial per workgroup; no atomics). */
size_t dasr_frame_ssd_u8_workspace(int B, int H, int W, int C, int crop);
int dasr_frame_ssd_u8(const unsigned char* a, const unsigned char* b, unsigned long long* ssd, void* workspace,
                      size_t workspace_bytes, int B, int H, int W, int C, int crop, void* stream);
/* dasr_image_metrics_u8: the four figures of the reference's test script (codes/test.py:97-152) for two uint8 [B,H,W,C]
 * image batches, C = 3 in BGR order (what dasr_frame_emit_u8 with swap_rb and cv2 produce) or C = 1, inside a crop-pixel
 * border (rows / columns crop .. H-1-crop / W-1-crop; crop == 0: the whole image, test.py:105-107).  With Hc = H - 2 crop,
 * Wc = W - 2 crop, per frame b:
 *   ssd[b]      exact (unsigned 64-bit) sum of (a - b)^2 over the region and all channels: dasr_frame_ssd_u8's quantity,
 *               the mse * count of calculate_psnr (utils/util.py:646-653)
 *   sums[b][0]  sum over the region of (Ya - Yb)^2, Y = (24.966 B + 128.553 G + 65.481 R) / 255 + 16 on the [0, 255] scale,
 *               not rounded: bgr2ycbcr(only_y=True) in its float branch (data/util.py:199-213; test.py:100-101 divides by
 *               255 first); 0 for C = 1
 *   sums[b][1]  sum of the SSIM map of utils/util.py:656-676 over its (Hc-10) x (Wc-10) x C positions (calculate_ssim,
 *               utils/util.py:679-697, averages three identical calls of ssim on the 3-channel array, and cv2.filter2D
 *               filters each channel by itself: the plain mean over positions and channels)
 *   sums[b][2]  the same sum for the one-channel luma image; 0 for C = 1
 * The SSIM map: window outer(k, k), k[i] = exp(-(i-5)^2 / (2 * 1.5^2)) normalised to sum 1 (cv2.getGaussianKernel(11, 1.5)),
 * correlation over VALID positions only, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, moments mu1, mu2, E[x^2] - mu1^2,
 * E[y^2] - mu2^2, E[xy] - mu1 mu2, map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)).  Luma,
 * moments, map and sums are fp64 (the window is applied separably).  This is NOT dasr_ssim's number (zero padding, fp32,
 * [0, 1] tensors).  PSNR = 20 log10(255 / sqrt(ssd / (Hc Wc C))), PSNR_Y likewise from sums[0] / (Hc Wc),
 * SSIM = sums[1] / ((Hc-10)(Wc-10) C), SSIM_Y = sums[2] / ((Hc-10)(Wc-10)).
 * C other than 1 or 3, Hc < 11 or Wc < 11: DASR_E_UNSUPPORTED (below 11 the reference's [5:-5] leaves an empty map and
 * returns NaN; that is refused, not reproduced).  B <= 65535.  workspace: dasr_image_metrics_u8_workspace() bytes, 8-byte
 * aligned (four partials per workgroup, added per frame in index order by a second launch; no atomics: a frame's result
 * has the same bits in every run, alone or as any member of a batch). */
size_t dasr_image_metrics_u8_workspace(int B, int H, int W, int C, int crop);
int dasr_image_metrics_u8(const unsigned char* a, const unsigned char* b, unsigned long long* ssd, double* sums,
                          void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int crop, void* stream);

/* ---- training batches from uint8 HR frames (csrc/batch.hip) --------------------------------------------------------
 * The image half of the reference's training loader (codes/data/LQGTker_Depth_dataset.py:145-199) on the device: the
 * uint8 HR frames cross PCIe, the LR image, the float GT, the augmentation and the NCHW RGB packing happen here.
 * Shared arguments: frames uint8 [B,H,W,3] HWC BGR; s the scale; (ch, cw) the size of the LR window (ch <= H/s,
 * cw <= W/s; the full frame: ch = H/s, cw = W/s); origins DEVICE int32 [B,2] = (oy, ox) of each sample's window in LR
 * pixels (NULL: all zero; values outside the frame are clamped into it); flags DEVICE uint8 [B], bit 0 hflip, bit 1
 * vflip, bit 2 transpose, applied in the order of augment (codes/data/util.py:101-118): img[:, ::-1], img[::-1],
 * transpose(1, 0, 2) (NULL: none).  allow_transpose != 0 says the flags may carry bit 2 and requires ch == cw
 * (DASR_E_SHAPE otherwise: a batch has one shape); with allow_transpose == 0 bit 2 is ignored.
 *
 * dasr_batch_lr_u8: lr float [B,3,ch,cw] NCHW RGB = the window of imresize_np(frames / 255, 1/s, antialiasing=True)
 * (codes/data/util.py:258-458: cubic, calculate_weights_indices, imresize_np; the division is read_img's,
 * codes/data/util.py:71-84), augmented.  Separable, H pass first, its result rounded to fp32; 4s taps per output;
 * symmetric edge-including reflection, applied by the kernel; not clamped, not rounded.  wh / ww: DEVICE float
 * [H/s, 4s] / [W/s, 4s] tap weights, ih / iw: DEVICE int32 [H/s] / [W/s] 0-based index of each output's first tap (may be
 * negative).  s in {2, 3, 4, 8} (DASR_E_UNSUPPORTED otherwise); H % s == 0, W % s == 0 and H, W >= floor(0.5 + 1.5 s),
 * the reflection length, below which the reference raises (DASR_E_SHAPE).  Each output is one fmaf chain in tap order:
 * its bits depend on neither the window, the batch nor the launch geometry. */
int dasr_batch_lr_u8(const unsigned char* frames, float* lr, const float* wh, const int* ih, const float* ww,
                     const int* iw, const int* origins, const unsigned char* flags, int B, int H, int W, int s, int ch,
                     int cw, int allow_transpose, void* stream);
/* dasr_batch_gt_u8: gt float [B,3,s*ch,s*cw] NCHW RGB = frames / 255 (IEEE division, the values of dasr_frame_ingest_u8;
 * read_img, codes/data/util.py:71-84) of the HR window at s * (oy, ox), augmented (codes/data/util.py:101-118) and packed
 * as LQGTker_Depth_dataset.py:186-193 does.  Any s > 0 with H % s == 0 and W % s == 0. */
int dasr_batch_gt_u8(const unsigned char* frames, float* gt, const int* origins, const unsigned char* flags, int B, int H,
                     int W, int s, int ch, int cw, int allow_transpose, void* stream);
/* dasr_batch_plane_f32 / _u8: in [B,C,h,w] -> out [B,C,ch,cw]: the window (oy, ox, ch, cw) of every plane, augmented
 * (codes/data/util.py:101-118 on the depth map and the mask list, LQGTker_Depth_dataset.py:176-193).  B * C <= 65535. */
int dasr_batch_plane_f32(const float* in, float* out, const int* origins, const unsigned char* flags, int B, int C, int h,
                         int w, int ch, int cw, int allow_transpose, void* stream);
int dasr_batch_plane_u8(const unsigned char* in, unsigned char* out, const int* origins, const unsigned char* flags, int B,
                        int C, int h, int w, int ch, int cw, int allow_transpose, void* stream);

/* ---- geometric self-ensemble inference (csrc/ensemble.hip) ------------------------------------------------------------
 * The reference's test_x8 (F_model_depthCond.py:236-270): the frame under the eight flip / transpose symmetries, each
 * result mapped back, the eight averaged.  Member m = v + 2 h + 4 t in the reference's list order: v flips along W (its
 * 'v', [:, :, :, ::-1]), h along H, t transposes last.  Members 0..3 are group A, images of H x W; members 4..7 group T,
 * images of W x H; member m of image n is image (m % 4) * N + n of its group's tensor.  With fh(r) = h ? H-1-r : r and
 * fv(c) = v ? W-1-c : c:   t = 0: x_m[n,r,c,:] = x[n,fh(r),fv(c),:]     t = 1: x_m[n,r,c,:] = x[n,fh(c),fv(r),:].
 * C must be 1 or 3 (DASR_E_UNSUPPORTED otherwise); N <= 65535.  No workspace, no atomics.
 *
 * dasr_ensemble_expand_f32 / _u8 (the `_transform` of F_model_depthCond.py:236-270 for all eight members): src [N,H,W,C]
 * -> out_a [4N,H,W,C], out_t [4N,W,H,C], a bit-exact move.  With C = 1 they take the depth map, the K mask planes
 * ([B,K,h,w] as N = B*K images: each member block is again [B,K,..]) and the region bytes (u8). */
int dasr_ensemble_expand_f32(const float* src, float* out_a, float* out_t, int N, int H, int W, int C, void* stream);
int dasr_ensemble_expand_u8(const unsigned char* src, unsigned char* out_a, unsigned char* out_t, int N, int H, int W,
                            int C, void* stream);
/* dasr_ensemble_ingest_u8 (F_model_depthCond.py:236-270 applied to a camera frame): dasr_frame_ingest_u8 followed by
 * dasr_ensemble_expand_f32 in one pass, bit for bit: every value is (float)byte / 255.0f (IEEE division); swap_rb != 0
 * with C == 3 reverses the channel order. */
int dasr_ensemble_ingest_u8(const unsigned char* frames, float* out_a, float* out_t, int N, int H, int W, int C,
                            int swap_rb, void* stream);
/* dasr_ensemble_merge (the inverse transforms and the mean of F_model_depthCond.py:236-270: i > 3 transpose, i % 4 > 1 h,
 * i % 2 == 1 v) with the output clamp of DepthNet.forward (sftmd_arch.py:950) applied to every member first: y_a
 * [4N,H,W,C], y_t [4N,W,H,C] are conv_output's results before the clamp;
 *   z_m[n,r,c,:] = clamp(y_m[n,fh(r),fv(c),:]) (t = 0),   clamp(y_m[n,fv(c),fh(r),:]) (t = 1),   clamp keeps NaN
 *   out[n,r,c,:] = 0.125f * (((((((z0 + z1) + z2) + z3) + z4) + z5) + z6) + z7), every addition rounded on its own. */
int dasr_ensemble_merge(const float* y_a, const float* y_t, float* out, int N, int H, int W, int C, float lo, float hi,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DASR_H */
