/*
 * fplx.h - C ABI of libfplx.so: the MI355X (gfx950 / CDNA4) hot path of FPL+
 * (3D U-Net with domain-specific BatchNorm: forward / backward, segmentation losses,
 * pseudo-label uncertainty filter, fused Adam).
 *
 * The reference (HiLab-git/FPL-plus) is pure Python and has no FFI; every device kernel it
 * runs comes from torch/ATen.  Each entry point below therefore cites the reference call
 * site (path under /root/reference/PyMIC/pymic unless noted) whose ATen op it replaces.
 *
 * Conventions
 *  - plain C: raw device pointers + sizes.  The CALLER owns every buffer (including
 *    workspaces); the library allocates nothing.  Its only mutable state is the table of
 *    integer tuning knobs behind fplx_set_tuning (A/B measurements; the defaults are the shipped
 *    configuration and every knob selects among kernels computing the same function - some in another order of fp32 additions, only which kernel computes it) and the calling
 *    thread's last error message.  The library never reads the environment.
 *  - only the functions declared here are exported (the library is built with
 *    -fvisibility=hidden; tests/test_host_cpu.py compares `nm -D` with this file).
 *  - activations are NDHWC ("channels last"): element (n,d,h,w,c) of a tensor with voxel
 *    stride `ld` (elements, >= C) lives at ((n*D+d)*H+h)*W+w)*ld + c.  ld > C addresses a
 *    channel slice of a wider buffer (the skip/up concat of UpBlock is never materialised).
 *  - `dt` selects the activation storage type: FPLX_F32 or FPLX_BF16.  Parameters,
 *    statistics, reductions and gradients of parameters are always fp32.
 *  - every launch is asynchronous on `stream` (a hipStream_t); no call synchronises.
 *  - return value: 0 on success, negative FPLX_E_* otherwise; fplx_last_error() gives the
 *    message of the calling thread's last failure.
 *  - reductions use fixed-order two-stage trees (no float atomics): bitwise reproducible.
 */
#ifndef FPLX_H
#define FPLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef void* fplx_stream_t; /* hipStream_t */

enum { FPLX_F32 = 0, FPLX_BF16 = 1 };

enum {
  FPLX_OK = 0,
  FPLX_E_BADSHAPE = -1,   /* unsupported / inconsistent shape            -> ValueError   */
  FPLX_E_BADDTYPE = -2,   /* unsupported dtype enum                      -> ValueError   */
  FPLX_E_WORKSPACE = -3,  /* workspace too small                         -> RuntimeError */
  FPLX_E_HIP = -4,        /* HIP launch error                            -> RuntimeError */
  FPLX_E_NULL = -5        /* required pointer is NULL                    -> ValueError   */
};

int fplx_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf; returns its length */
int fplx_last_error(char* buf, size_t n);
/* number of partial-sum rows the reduction kernels write for a tensor of `voxels` voxels */
int fplx_num_partials(int64_t voxels);

/* ------------------------------------------------------------------ tuning knobs and plan queries
 * (no reference counterpart: the reference's kernels are cuDNN's, chosen by torch.backends.cudnn.benchmark,
 *  agent_seg.py:737-738 sets deterministic = True / benchmark = False)
 * fplx_set_tuning / fplx_get_tuning: named integer knobs that select among equivalent kernels / launch geometries
 *   ("xcd", "brick", "march", "march32_v2", "wg_cot", "tile_ks", ...; fplx_tuning_key enumerates them: returns the key's
 *   length and copies it, or -1 past the end).  Unknown key: FPLX_E_BADSHAPE.  Benchmarks and tests only.
 * fplx_conv3d_plan_query: which kernel family fplx_conv3d_fwd dispatches this layer to (for 16-byte aligned NDHWC bf16
 *   operands; FPLX_KERNEL_*), the geometry (brick: 0 = 4x8x8, 1 = 5x4x8; depth march: Cin = 32: 2 = the one-wave-per-SIMD
 *   kernels for footprints inside the volume [statistics form / statistics-free form], 0 = the 8-wave kernel; Cin >= 64: the
 *   footprint width 16 | 32; -1 for other families), the split of the reduction dimension (1 = none) and the statistics
 *   rows - pure host code, no launch.  FPLX_KERNEL_STREAM is reserved: its kernel has been removed, no query returns it,
 *   and the other values keep their numbers. */
enum {
  FPLX_KERNEL_GENERIC = 0, FPLX_KERNEL_DIRECT = 1, FPLX_KERNEL_TILE = 2, FPLX_KERNEL_STREAM = 3, FPLX_KERNEL_MARCH = 4,
  FPLX_KERNEL_BRICK = 5, FPLX_KERNEL_STEM = 6, FPLX_KERNEL_OUTCONV = 7
};
int fplx_set_tuning(const char* key, int64_t value);
int fplx_get_tuning(const char* key, int64_t* value);
int fplx_tuning_key(int index, char* buf, size_t n);
int fplx_conv3d_plan_query(int n, int d, int h, int w, int cin, int cout, int kd, int kh, int kw, int x_dt, int y_dt,
                           int* kernel, int* geometry, int* ksplit, int* stats_rows);

/* ------------------------------------------------------------------ weight packing
 * nn.Conv3d weight [Cout][Cin][KD][KH][KW] fp32 (net/net3d/unet2d5_dsbn.py:54-55, 293-294)
 *   -> wf[tap][Cout][Cin]  (forward operand)
 *   -> wb[tap][Cin][Cout]  with tap mirrored (data-gradient operand; may be NULL)
 * both in dtype dt.  tap = (kd*KH + kh)*KW + kw. */
int fplx_pack_conv_weight(const float* w, void* wf, void* wb, int cout, int cin, int kd, int kh, int kw,
                          int dt, fplx_stream_t stream);
/* the same for n (<= 32) 3x3x3 layers in one launch: host arrays of per-layer pointers / channel counts (what the train
 * step does after every optimizer step for all ConvBlockND convolutions, unet2d5_dsbn.py:54-55).  wb[i] may be NULL.
 * stamp (may be NULL; layers with cout % 16 == 0 and cin % 32 == 0 in bf16 only): stamp[i] = caller-owned buffer of
 * (cout / 16) * (cin / 32) * 32 floats per layer (or NULL) that receives, per 16 x 32-channel pack tile, 32 of the fp32 master
 * values the tile's pack was made from.  verify = 1: the packs and stamps of an earlier call (or of fplx_adam_pack_step) are
 * still in wf / wb / stamp - only the tiles whose masters no longer match their stamps bit for bit are packed again.  This is
 * how a caller that keeps packs across optimiser steps notices writers that bypass it (torch's `.data` edits bump no version
 * counter: agent_seg.py's EMA / init paths); whole-tensor writes are always caught, single-element edits between the sampled
 * positions (elements 0 and 432 of every 864-element row segment) are not. */
int fplx_pack_conv_weights_batched(int n, const float* const* w, void* const* wf, void* const* wb, const int* cout,
                                   const int* cin, int dt, float* const* stamp, int verify, fplx_stream_t stream);
/* n (<= 16) small packs in one launch: job i is a convolution weight [a][b][taps] fp32 (kind 0: a = Cout, b = Cin, layouts of
 * fplx_pack_conv_weight) or a transposed-convolution weight (kind 1: a = Cin, b = Cout, layouts of fplx_pack_deconv_weight /
 * _deconv122_weight) packed into wf[i] / wb[i] (either may be NULL) in dtype dt[i] - the stem, the four transposed convolutions
 * and out_conv of the network (unet2d5_dsbn.py:54, 152, 293): what a train step otherwise launches one by one after Adam */
int fplx_pack_weights_multi(int n, const int* kind, const float* const* w, void* const* wf, void* const* wb, const int* a,
                            const int* b, const int* taps, const int* dt, fplx_stream_t stream);
/* nn.ConvTranspose3d weight [Cin][Cout][2][2][2] fp32 (unet2d5_dsbn.py:152)
 *   -> wf[tap][Cout][Cin] and wb[tap][Cin][Cout] (dtype dt), tap = (i*2+j)*2+k */
int fplx_pack_deconv_weight(const float* w, void* wf, void* wb, int cin, int cout, int dt,
                            fplx_stream_t stream);

/* ------------------------------------------------------------------ convolution
 * Generic "same" convolution, stride 1, zero padding (KD/2, KH/2, KW/2):
 *   nn.Conv3d(k=3,p=1)            unet2d5_dsbn.py:54-55 used at 75,79
 *   nn.Conv3d(k=(1,3,3),p=(0,1,1)) unet2d5_dsbn.py:293-294, 307 (out_conv)
 * and, with the mirrored pack `wb`, the data gradient of either.
 *  x      input, described by explicit element strides (sn,sd,sh,sw,sc) so that both the
 *         fp32 NCDHW network input and NDHWC activations can be read; type x_dt
 *  wp     packed weight [taps][Cout][Cin], type = y's dt for NDHWC outputs, fp32 otherwise
 *  bias   fp32 [Cout] or NULL
 *  y      output, element strides (yn,yd,yh,yw,yc), type y_dt
 *         (i.e. the packed weight has the type of y)
 *  stats  optional fp32 [fplx_conv3d_stats_rows(...)][2][Cout]: per-row sum / sum of squares of
 *         the (unrounded) outputs, for the BatchNorm that follows (dsbn.py:54-57).  The row
 *         count depends on the kernel variant chosen for the shape; ask for it. */
int fplx_conv3d_stats_rows(int n, int d, int h, int w, int cin, int cout, int kd, int kh, int kw, int x_dt, int y_dt);
/*  ws     workspace of fplx_conv3d_fwd_ws_bytes(...) bytes (0 for most shapes; small deep-level volumes
 *         use a split-K kernel that keeps fp32 partial tiles there).  ws may be NULL when that is 0. */
size_t fplx_conv3d_fwd_ws_bytes(int n, int d, int h, int w, int cin, int cout, int kd, int kh, int kw, int x_dt, int y_dt);
int fplx_conv3d_fwd(const void* x, int x_dt, int64_t sn, int64_t sd, int64_t sh, int64_t sw, int64_t sc,
                    const void* wp, const float* bias,
                    void* y, int y_dt, int64_t yn, int64_t yd, int64_t yh, int64_t yw, int64_t yc,
                    int n, int d, int h, int w, int cin, int cout, int kd, int kh, int kw,
                    float* stats, void* ws, size_t ws_bytes, fplx_stream_t stream);

/* weight + bias gradient of the same convolution.
 *  dw   fp32 [Cout][Cin][KD][KH][KW] (torch layout), db fp32 [Cout] or NULL
 *  ws   workspace of at least fplx_conv3d_wgrad_ws_bytes(...) bytes */
size_t fplx_conv3d_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout, int kd, int kh, int kw);
int fplx_conv3d_wgrad(const void* x, int x_dt, int64_t sn, int64_t sd, int64_t sh, int64_t sw, int64_t sc,
                      const void* dy, int dy_dt, int64_t yn, int64_t yd, int64_t yh, int64_t yw, int64_t yc,
                      float* dw, float* db, int n, int d, int h, int w, int cin, int cout,
                      int kd, int kh, int kw, void* ws, size_t ws_bytes, fplx_stream_t stream);

/* The stem site's weight gradient fused with the apply pass of its BatchNorm + PReLU backward (round 6).  The gradient w.r.t.
 * the output of the network's first convolution (Conv3d(in_chns -> C0), unet2d5_dsbn.py:54, 74-77) has one consumer - this
 * weight gradient; the network input needs no data gradient - so fplx_bn_act_bwd_apply + fplx_conv3d_wgrad of that site (write dy,
 * read it back) become one call: y = the convolution's stored output (bf16 [V, ldy]), dout = gradient w.r.t. the site's output a
 * (bf16 [V, ldd]), mean .. slope = the site's BatchNorm constants, coef = fplx_bn_act_bwd_finalize's; the kernel forms
 * dy = scale (dz - k0 - x-hat k1) -> bf16 on the pieces it stages (fplx_bn_act_bwd_apply's arithmetic, dropout-free) and dy is
 * never stored.  x: fp32 NCDHW contiguous, in_chns 1 | 4, C0 % 32 == 0 (fplx_conv3d_plan_query answers FPLX_KERNEL_STEM for the
 * forward); dw, ws as fplx_conv3d_wgrad with ws of fplx_conv3d_wgrad_ws_bytes(.., 3, 3, 3) bytes.  dw is bit for bit the
 * two-call result. */
int fplx_stem_wgrad_bn(const float* x, const void* y, int64_t ldy, const void* dout, int64_t ldd, const float* mean,
                       const float* rstd, const float* scale, const float* shift, const float* slope, const float* coef,
                       float* dw, int n, int d, int h, int w, int cin, int cout, void* ws, size_t ws_bytes, fplx_stream_t stream);

/* The first convolution of an UpBlock reads torch.cat([skip, up], dim=1) (unet2d5_dsbn.py:182-183).  Where the two
 * halves are 32 channels wide (level 0) a concat BUFFER would be addressed in half 128-byte lines by every other
 * kernel that touches one half (pooling, transposed convolution), so there the concatenation is never built: these
 * three entry points take / produce the two tensors separately (bf16 NDHWC, both with leading dimension ldx;
 * cin = total input channels = 64).  fplx_conv3d_cat2_ok tells whether a shape is served; stats rows and the
 * workspace size are those of fplx_conv3d_stats_rows / fplx_conv3d_wgrad_ws_bytes for the same (cin, cout). */
int fplx_conv3d_cat2_ok(int n, int d, int h, int w, int cin, int cout);
int fplx_conv3d_fwd_cat2(const void* x0, const void* x1, int64_t ldx, const void* wp, const float* bias, void* y,
                         int64_t ldy, int n, int d, int h, int w, int cin, int cout, float* stats,
                         fplx_stream_t stream);
/* dy: [voxels][cout]; wb: the mirrored pack of the same weight; dx0 / dx1: gradients of the two input halves */
int fplx_conv3d_dgrad_split2(const void* dy, int64_t ldy, const void* wb, void* dx0, void* dx1, int64_t ldx, int n,
                             int d, int h, int w, int cin, int cout, fplx_stream_t stream);
int fplx_conv3d_wgrad_cat2(const void* x0, const void* x1, int64_t ldx, const void* dy, int64_t ldy, float* dw, int n,
                           int d, int h, int w, int cin, int cout, void* ws, size_t ws_bytes, fplx_stream_t stream);

/* ------------------------------------------------------------------ inference: convolution + BatchNorm(eval) + PReLU in one kernel
 * ConvBlockND in eval mode (unet2d5_dsbn.py:74-81 with dsbn.py:54-57 on running statistics): BatchNorm is then a fixed
 * per-channel affine map, z = scale (conv(x; w) + b) + shift = conv(x; scale w) + (scale b + shift).  The CALLER folds scale
 * into the weights before packing them (fplx_pack_conv_weight / _conv2d_weight) and passes bias = scale b + shift; the
 * kernel applies PReLU(prelu_slope[0]) in its write-out, so the separate fplx_bn_act_fwd pass disappears.  bf16 NDHWC
 * operands, 3x3x3 (mid != 0: a Conv2d pack in the middle depth plane).  x1 != NULL: the input is cat([x0, x1], channel)
 * of two cin/2-channel tensors (as fplx_conv3d_fwd_cat2; here also the brick kernel's layers, e.g. 64 || 64 -> 64 at level
 * 1).  Only for layers fplx_conv3d_fwd_act_ok accepts (the depth-march,
 * brick and split-K kernels); FPLX_E_BADSHAPE otherwise - callers fall back to fplx_conv3d_fwd + fplx_bn_act_fwd.
 * n_x0 (two-tensor form only; 0 = n): x0 holds n_x0 samples and sample i reads x0[i % n_x0] - the Monte-Carlo passes of
 * test-time dropout (agent_seg.py:898-909) share the encoder levels above the first active dropout, whose skip tensor is
 * then not replicated per pass.  ws: fplx_conv3d_fwd_ws_bytes / fplx_conv2d_fwd_ws_bytes of the layer. */
int fplx_conv3d_fwd_act_ok(int n, int d, int h, int w, int cin, int cout, int mid, int cat2);
int fplx_conv3d_fwd_act(const void* x0, const void* x1, int64_t ldx, const void* wp, const float* bias,
                        const float* prelu_slope, void* y, int64_t ldy, int n, int d, int h, int w, int cin, int cout,
                        int mid, int n_x0, void* ws, size_t ws_bytes, fplx_stream_t stream);

/* ------------------------------------------------------------------ transposed convolution
 * nn.ConvTranspose3d(k=2,s=2) (unet2d5_dsbn.py:152,181).  x: [N,D,H,W,Cin] ld ldx;
 * y: [N,2D,2H,2W,Cout] ld ldy (normally the upper channel half of the concat buffer, line 182). */
int fplx_deconv2_fwd(const void* x, int64_t ldx, const void* wf, const float* bias, void* y, int64_t ldy,
                     int n, int d, int h, int w, int cin, int cout, int dt, fplx_stream_t stream);
int fplx_deconv2_dgrad(const void* dy, int64_t ldy, const void* wb, void* dx, int64_t ldx,
                       int n, int d, int h, int w, int cin, int cout, int dt, fplx_stream_t stream);
size_t fplx_deconv2_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout);
/* dw fp32 [Cin][Cout][2][2][2], db fp32 [Cout] */
int fplx_deconv2_wgrad(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, float* db,
                       int n, int d, int h, int w, int cin, int cout, int dt,
                       void* ws, size_t ws_bytes, fplx_stream_t stream);

/* ------------------------------------------------------------------ 2.5D levels (conv_dims[l] = 2, the shipped configs:
 * config_dual/data_vs/vs_t1s_g.cfg:58 conv_dims = [2, 2, 3, 3, 3]).  The reference folds the depth axis into the batch and
 * runs 2D modules (unet2d5_dsbn.py:110-127, 160-188); on [N,D,H,W,C] volumes that is
 *  - Conv2d(3x3, pad 1)  = the 3x3x3 kernels with the 9 taps packed into the middle depth plane (pack_conv2d_weight:
 *    w fp32 [Cout][Cin][3][3] -> the same wf / wb layouts as fplx_pack_conv_weight); weight gradient = middle plane of
 *    the 27-tap gradient (dw27 [Cout][Cin][27] -> dw9 [Cout][Cin][9], taps 9..17)
 *  - MaxPool2d(2)        = maxpool122: x [N,D,H,W,C] -> y [N,D,H/2,W/2,C]
 *  - ConvTranspose2d(2,2) = deconv122: x [N,D,H,W,Cin] -> y [N,D,2H,2W,Cout]; weights fp32 [Cin][Cout][2][2] packed to
 *    wf [4][Cout][Cin], wb [4][Cin][Cout]; dw fp32 [Cin][Cout][2][2]
 *  BatchNorm2d over (N D, C, H, W) has the statistics of BatchNorm3d over (N, C, D, H, W): same kernels.
 *  fplx_conv2d_* = fplx_conv3d_* (3x3x3) for such packs, same arguments and results; knowing that only the middle plane
 *  is live, the implicit-GEMM kernel runs 9 taps instead of 27. */
int fplx_pack_conv2d_weight(const float* w, void* wf, void* wb, int cout, int cin, int dt, fplx_stream_t stream);
int fplx_conv2d_stats_rows(int n, int d, int h, int w, int cin, int cout, int x_dt, int y_dt);
size_t fplx_conv2d_fwd_ws_bytes(int n, int d, int h, int w, int cin, int cout, int x_dt, int y_dt);
int fplx_conv2d_fwd(const void* x, int x_dt, int64_t sn, int64_t sd, int64_t sh, int64_t sw, int64_t sc,
                    const void* wp, const float* bias, void* y, int y_dt, int64_t yn, int64_t yd, int64_t yh,
                    int64_t yw, int64_t yc, int n, int d, int h, int w, int cin, int cout,
                    float* stats, void* ws, size_t ws_bytes, fplx_stream_t stream);
int fplx_conv2d_fwd_cat2(const void* x0, const void* x1, int64_t ldx, const void* wp, const float* bias, void* y,
                         int64_t ldy, int n, int d, int h, int w, int cin, int cout, float* stats,
                         fplx_stream_t stream);                     /* = fplx_conv3d_fwd_cat2 for such packs */
int fplx_conv2d_dgrad_split2(const void* dy, int64_t ldy, const void* wb, void* dx0, void* dx1, int64_t ldx, int n,
                             int d, int h, int w, int cin, int cout, fplx_stream_t stream);
/* weight gradient of the Conv2d: dw fp32 [Cout][Cin][3][3], db fp32 [Cout] or NULL (9 of 27 taps on the MFMA path) */
size_t fplx_conv2d_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout);
int fplx_conv2d_wgrad(const void* x, int x_dt, int64_t sn, int64_t sd, int64_t sh, int64_t sw, int64_t sc,
                      const void* dy, int dy_dt, int64_t yn, int64_t yd, int64_t yh, int64_t yw, int64_t yc,
                      float* dw, float* db, int n, int d, int h, int w, int cin, int cout,
                      void* ws, size_t ws_bytes, fplx_stream_t stream);
int fplx_conv2d_wgrad_cat2(const void* x0, const void* x1, int64_t ldx, const void* dy, int64_t ldy, float* dw, int n,
                           int d, int h, int w, int cin, int cout, void* ws, size_t ws_bytes, fplx_stream_t stream);
int fplx_maxpool122_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, int n, int d, int h, int w, int c,
                        int dt, fplx_stream_t stream);
int fplx_maxpool122_bwd(const void* x, int64_t ldx, const void* dy, int64_t ldy, const void* dskip, int64_t lds,
                        void* dx, int64_t ldo, int n, int d, int h, int w, int c, int dt, fplx_stream_t stream);
int fplx_pack_deconv122_weight(const float* w, void* wf, void* wb, int cin, int cout, int dt, fplx_stream_t stream);
int fplx_deconv122_fwd(const void* x, int64_t ldx, const void* wf, const float* bias, void* y, int64_t ldy,
                       int n, int d, int h, int w, int cin, int cout, int dt, fplx_stream_t stream);
int fplx_deconv122_dgrad(const void* dy, int64_t ldy, const void* wb, void* dx, int64_t ldx,
                         int n, int d, int h, int w, int cin, int cout, int dt, fplx_stream_t stream);
size_t fplx_deconv122_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout);
int fplx_deconv122_wgrad(const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw, float* db,
                         int n, int d, int h, int w, int cin, int cout, int dt,
                         void* ws, size_t ws_bytes, fplx_stream_t stream);

/* ------------------------------------------------------------------ DSBN + PReLU + dropout
 * Training-mode statistics of nn.BatchNorm3d for the ACTIVE domain (dsbn.py:54-57):
 *   stats [rows][2][C] (from fplx_conv3d_fwd) -> mean, biased var -> scale = gamma*rstd,
 *   shift = beta - mean*scale; running_mean/var updated with momentum (unbiased var),
 *   num_batches_tracked += 1 (int64, may be NULL).  eps as torch (1e-5). */
int fplx_bn_train_finalize(const float* stats, int rows, int c, int64_t count,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps,
                           float* mean, float* rstd, float* scale, float* shift, fplx_stream_t stream);
/* Statistics of an NDHWC tensor for a stand-alone DomainSpecificBatchNorm3d call (dsbn.py:54-57):
 * stats fp32 [fplx_num_partials(voxels)][2][C], same format fplx_conv3d_fwd emits. */
int fplx_channel_stats(const void* x, int64_t ldx, int64_t voxels, int c, int dt, float* stats,
                       fplx_stream_t stream);
/* Eval mode: scale/shift from the running statistics. */
int fplx_bn_eval_prepare(const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, int c, float* scale, float* shift,
                         fplx_stream_t stream);
/* out = dropout_p(PReLU_slope(y*scale + shift))   (unet2d5_dsbn.py:76-78 / 80-81)
 * dropout keep-mask = counter-based Philox stream (seed, stream_id, flat NDHWC index of `out`
 * assuming ld == C numbering); p == 0 disables it.  y and out may alias. */
int fplx_bn_act_fwd(const void* y, int64_t ldy, void* out, int64_t ldo, const float* scale, const float* shift,
                    const float* slope, float p, uint64_t seed, uint32_t stream_id,
                    int64_t voxels, int c, int dt, fplx_stream_t stream);
/* Backward, stage 1: partial sums over voxels of dz and dz*xhat per channel and of the PReLU
 * slope gradient: part [rows][2*C+1] (rows = fplx_num_partials(voxels)). */
int fplx_bn_act_bwd_reduce(const void* y, int64_t ldy, const void* dout, int64_t ldd,
                           const float* mean, const float* rstd, const float* scale, const float* shift,
                           const float* slope, float p, uint64_t seed, uint32_t stream_id,
                           int64_t voxels, int c, int dt, float* part, fplx_stream_t stream);
/* stage 2: dgamma, dbeta (ACCUMULATED into the fp32 grads), dslope (accumulated), and the
 * two per-channel coefficients coef[2][C] used by stage 3.  train=0: eval-mode BN (statistics
 * are constants): coefficients are zero. */
int fplx_bn_act_bwd_finalize(const float* part, int rows, int c, int64_t count, int train,
                             float* dgamma, float* dbeta, float* dslope, float* coef, fplx_stream_t stream);
/* stage 3: dy = gamma*rstd * (dz - coef0 - xhat*coef1).  dy may alias dout. */
int fplx_bn_act_bwd_apply(const void* y, int64_t ldy, const void* dout, int64_t ldd, void* dy, int64_t ldo,
                          const float* mean, const float* rstd, const float* scale, const float* shift,
                          const float* slope, const float* coef, float p, uint64_t seed, uint32_t stream_id,
                          int64_t voxels, int c, int dt, fplx_stream_t stream);

/* ------------------------------------------------------------------ pooling
 * nn.MaxPool3d(2,2) (unet2d5_dsbn.py:106,117).  x [N,D,H,W,C] ld ldx -> y [N,D/2,H/2,W/2,C] ld ldy */
int fplx_maxpool2_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, int n, int d, int h, int w, int c,
                      int dt, fplx_stream_t stream);
/* dx = dskip (may be NULL) + scatter(dy to the first maximum of each 2x2x2 window of x) */
int fplx_maxpool2_bwd(const void* x, int64_t ldx, const void* dy, int64_t ldy, const void* dskip, int64_t lds,
                      void* dx, int64_t ldo, int n, int d, int h, int w, int c, int dt, fplx_stream_t stream);

/* Fused tail of a DownBlock (second ConvBlockND site - no dropout there - then the pooling, unet2d5_dsbn.py:79-81, 117):
 *  fplx_bn_act_pool_fwd:   a2 = PReLU(BN(y2)) written to `out` (the skip tensor) and MaxPool(a2) to `pooled` in one pass.
 *  fplx_pool_bwd_bn_reduce: dx = dskip + unpooled(dy) = d(a2) (first-maximum rule on a2 recomputed from y2) and, over that
 *                          dx, the partial rows of fplx_bn_act_bwd_reduce for this site (same layout: fplx_num_partials(voxels)
 *                          rows of 2C+1 floats) - the caller then runs fplx_bn_act_bwd_finalize / _apply as usual.
 * pd = 2: MaxPool3d(2), pd = 1: MaxPool2d(2) per depth slice; dims = the UNPOOLED tensor's; bf16 only, see fplx_bn_pool_fused_ok. */
int fplx_bn_pool_fused_ok(int c, int dt);
int fplx_bn_act_pool_fwd(const void* y, int64_t ldy, void* out, int64_t ldo, void* pooled, int64_t ldp, const float* scale,
                         const float* shift, const float* slope, int n, int d, int h, int w, int c, int dt, int pd,
                         fplx_stream_t stream);
int fplx_pool_bwd_bn_reduce(const void* y, int64_t ldy, const void* dy, int64_t lddy, const void* dskip, int64_t lds, void* dx,
                            int64_t ldo, const float* mean, const float* rstd, const float* scale, const float* shift,
                            const float* slope, int n, int d, int h, int w, int c, int dt, int pd, float* part,
                            fplx_stream_t stream);

/* out_conv (Conv3d C0 -> classes, kernel (1,3,3), unet2d5_dsbn.py:293-294, 307) fused with the BatchNorm + PReLU passes of the
 * convolution site in front of it (ConvBlockND's second site of the last UpBlock, unet2d5_dsbn.py:79-81; dropout-free, bf16
 * NDHWC, C0 = 32, classes <= 4: fplx_outconv_bn_rows > 0).  The out_conv operands are 1 / 8 the size of that site's tensors, so
 *   fplx_outconv_fwd_bn          reads the site's PRE-BatchNorm output y, applies a = PReLU(scale y + shift) on the way into its
 *                                tiles, writes a (unless NULL, see below) and the fp32 planar logits: fplx_bn_act_fwd + fplx_conv3d_fwd
 *                                in one pass over y; a and the logits are the bits of the two-call path;
 *   fplx_outconv_dgrad_bn_reduce / _apply   never store out_conv's data gradient: both RECOMPUTE it from dlogits (fp32 planar)
 *                                and the mirrored pack wb and run fplx_bn_act_bwd_reduce / _apply on it - _reduce writes
 *                                fplx_outconv_bn_rows(...) partial rows of 2 C0 + 1 floats for fplx_bn_act_bwd_finalize,
 *                                _apply takes the finalize's coef and writes dy (gradient w.r.t. y);
 *   fplx_outconv_wgrad_bn        out_conv's weight gradient dw [classes][C0][1][3][3] and bias gradient db [classes] (NULL: not
 *                                wanted) from y as well: a is formed on the way in, exactly as fplx_outconv_fwd_bn forms it.
 *                                With the three of them a has no reader left in a training step, and fplx_outconv_fwd_bn takes
 *                                a = NULL (no activation written) wherever fplx_outconv_wgrad_bn_ws_bytes(...) > 0 - classes <= 3;
 *                                0 = this form is not available, a is required and fplx_conv3d_wgrad takes the gradient from it.
 *                                ws: fplx_outconv_wgrad_bn_ws_bytes(...) bytes.  dw agrees with fplx_conv3d_wgrad on the stored a
 *                                to fp32 summation order (same bf16 operands).
 * mean / rstd / scale / shift: the site's BatchNorm constants (fplx_bn_train_finalize / fplx_bn_eval_prepare). */
/* partial rows the fused backward writes, or 0 where the fused forms do not apply (the caller then runs the separate passes) */
int fplx_outconv_bn_rows(int n, int d, int h, int w, int c0, int ncls);
int fplx_outconv_fwd_bn(const void* y, int64_t ldy, const float* scale, const float* shift, const float* prelu_slope, void* a,
                        int64_t lda, const float* wf, const float* bias, float* logits, int n, int d, int h, int w, int c0,
                        int ncls, fplx_stream_t stream);
int fplx_outconv_dgrad_bn_reduce(const float* dlogits, const void* wb, const void* y, int64_t ldy, const float* mean,
                                 const float* rstd, const float* scale, const float* shift, const float* prelu_slope,
                                 float* part, int n, int d, int h, int w, int c0, int ncls, fplx_stream_t stream);
int fplx_outconv_dgrad_bn_apply(const float* dlogits, const void* wb, const void* y, int64_t ldy, const float* mean,
                                const float* rstd, const float* scale, const float* shift, const float* prelu_slope,
                                const float* coef, void* dy, int64_t lddy, int n, int d, int h, int w, int c0, int ncls,
                                fplx_stream_t stream);
size_t fplx_outconv_wgrad_bn_ws_bytes(int n, int d, int h, int w, int c0, int ncls);
int fplx_outconv_wgrad_bn(const void* y, int64_t ldy, const float* scale, const float* shift, const float* prelu_slope,
                          const float* dlogits, float* dw, float* db, int n, int d, int h, int w, int c0, int ncls, void* ws,
                          size_t ws_bytes, fplx_stream_t stream);

/* (Tri / bi)linear x2 upsampling, align_corners = True - UpBlock with bilinear = True (unet2d5_dsbn.py:148-150, 172-176:
 * nn.Upsample(scale_factor=2, mode='trilinear' | 'bilinear', align_corners=True) behind a kernel-1 convolution, which runs
 * through fplx_conv3d_fwd / _wgrad with kd = kh = kw = 1).  x [n][d][h][w][ldx] -> y [n][sd*d][2h][2w][ldy]; sd = 2:
 * trilinear, sd = 1: bilinear on every depth slice (2.5D levels).  bwd: dx = the transpose applied to dy (gather, no atomics). */
int fplx_upsample2_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, int n, int d, int h, int w, int c, int dt, int sd,
                       fplx_stream_t stream);
int fplx_upsample2_bwd(const void* dy, int64_t ldy, void* dx, int64_t ldx, int n, int d, int h, int w, int c, int dt, int sd,
                       fplx_stream_t stream);

/* ------------------------------------------------------------------ 1x1x1 classification head + deep-supervision interpolation
 * (csrc/head.hip) UNet3D's out_conv and out_conv1..3 (PyMIC/pymic/net/net3d/unet3d.py:131-135) and the interpolate(...,
 * mode='trilinear') that brings a coarse head's logits to full size (unet3d.py:152-158).
 * a: NDHWC activation [n * v][lda] of dtype dt (lda >= c; rows 16-byte aligned: lda % 4 == 0 for fp32, % 8 for bf16 - lda = 2 c
 * where a is the left half of a concat buffer); w fp32 [ncls][c]; bias fp32 [ncls] (may be NULL: zero); logits / dlogits fp32
 * planar [n][ncls][v].  c: a multiple of 8 up to 512; 1 <= ncls <= 8.  Anything else: FPLX_E_BADSHAPE / _BADDTYPE / _NULL before
 * any launch.  All sums in a fixed order, no atomics.
 *   fwd     logits[n][k][v] = bias[k] + sum_c w[k][c] a[n][v][c], fp32, c ascending
 *   dgrad   da[n][v][c] = sum_k w[k][c] dlogits[n][k][v] (k ascending), rounded to dt; accumulate != 0: da = da + that, in place
 *   wgrad   dw[k][c] = sum_{n,v} dlogits a, db[k] = sum dlogits (db may be NULL); two stages through ws of
 *           fplx_head_wgrad_ws_bytes(n, v, c, ncls) bytes (0: shape refused); too small: FPLX_E_WORKSPACE */
int fplx_head_fwd(const void* a, int64_t lda, int dt, const float* w, const float* bias, float* logits, int n, int64_t v, int c,
                  int ncls, fplx_stream_t stream);
int fplx_head_dgrad(const float* dlogits, const float* w, void* da, int64_t lda, int dt, int n, int64_t v, int c, int ncls,
                    int accumulate, fplx_stream_t stream);
size_t fplx_head_wgrad_ws_bytes(int n, int64_t v, int c, int ncls);
int fplx_head_wgrad(const void* a, int64_t lda, int dt, const float* dlogits, float* dw, float* db, int n, int64_t v, int c,
                    int ncls, void* ws, size_t ws_bytes, fplx_stream_t stream);
/* Trilinear interpolation, align_corners = False, by one integer factor f in {2, 4, 8} on all three axes (other factors:
 * FPLX_E_BADSHAPE): x fp32 planar [nc][d][h][w] -> y [nc][f d][f h][f w].  ATen's rule: src = max((dst + 0.5) / f - 0.5, 0),
 * upper neighbour clamped at the edge.  bwd: dx = the exact transpose applied to dy, as a gather in a fixed order (no atomics). */
int fplx_interp_fwd(const float* x, float* y, int64_t nc, int d, int h, int w, int f, fplx_stream_t stream);
int fplx_interp_bwd(const float* dy, float* dx, int64_t nc, int d, int h, int w, int f, fplx_stream_t stream);

/* ------------------------------------------------------------------ segmentation loss
 * Fused softmax + Dice (loss/seg/dice.py:20-57, util.py:85-107) + cross entropy
 * (loss/seg/ce.py:23-44) + per-sample image-weighted Dice (dice.py:106-128) + entropy
 * regulariser (net_run_dsbn/agent_seg.py:352-354) + hard-Dice train metric
 * (agent_seg.py:472-476).  logits / label: fp32 [N,C,D,H,W] contiguous (1 <= C <= 8, N <= 64);
 * pixel_weight fp32 [N,1,D,H,W] or NULL.
 *   softmax  1: Dice and CE take softmax(logits); 0: they take the outputs as they are (loss_softmax = False, the outputs are
 *          probabilities).  The entropy regulariser applies softmax to the outputs in BOTH cases, as the reference does
 *          (agent_seg.py:353 `outputs.softmax(1)`): with softmax = 0 its value and gradient still go through softmax(logits),
 *          and the hard-Dice metric takes the first maximum of the raw outputs either way.
 *   part   fp32 workspace [N][rows][FPLX_LOSS_K(C)], rows = fplx_loss_rows(D*H*W) (partial rows + 5 spare rows that hold the
 *          per-sample sums and batch totals as (N + 1) x K doubles, 8-byte aligned: exactly N*rows*K floats are touched)
 *   cfg    host floats: w_dice, w_ce, w_dice_img (per-sample Dice x image_weight), w_entropy
 *   image_weight fp32 [N] device or NULL (needed iff w_dice_img != 0)
 *   out    fp32 device [4 + C]: total loss, dice term, ce term, entropy term, hard class Dice[C]
 *   coef   fp32 device [N][C][2] + [2]: backward coefficients (written by the finalize kernel)
 * Data parallelism (one process per GPU): the reference's nn.DataParallel gathers the replicas' logits and evaluates ONE
 * loss over the full batch (agent_seg.py:692-698 with get_loss_value 134-142); Dice and the weighted CE are not sums of
 * per-shard losses.  fplx_seg_loss_fwd = fplx_seg_loss_sums + fplx_seg_loss_from_sums; between the two a caller
 * all-reduces `totals` (double [FPLX_LOSS_K(C)], the sums over the local samples) over the ranks and passes the global
 * sample count: loss value, metric and coefficients are then those of the full batch, and the ranks' gradients ADD UP to
 * the full-batch gradient (no division by the world size).
 *   sums   double device [N][FPLX_LOSS_K(C)] per-sample sums;  totals double device [FPLX_LOSS_K(C)] */
#define FPLX_LOSS_K(C) (6 * (C) + 3)
int fplx_loss_rows(int64_t voxels_per_sample);
int fplx_seg_loss_fwd(const float* logits, const float* label, const float* pixel_weight,
                      const float* image_weight, int n, int c, int64_t voxels_per_sample,
                      float w_dice, float w_ce, float w_dice_img, float w_entropy, int softmax,
                      float* part, float* out, float* coef, fplx_stream_t stream);
int fplx_seg_loss_sums(const float* logits, const float* label, const float* pixel_weight, int n, int c,
                       int64_t voxels_per_sample, int softmax, float* part, double* sums, double* totals,
                       fplx_stream_t stream);
int fplx_seg_loss_from_sums(const double* sums, const double* totals, const float* image_weight, int n, int n_global, int c,
                            int64_t voxels_per_sample, int has_pixel_weight, float w_dice, float w_ce, float w_dice_img,
                            float w_entropy, float* out, float* coef, fplx_stream_t stream);
/* dlogits = gscale[0] * dLoss/dlogits ; gscale: device fp32 scalar (upstream gradient) */
int fplx_seg_loss_bwd(const float* logits, const float* label, const float* pixel_weight,
                      const float* coef, const float* gscale, int n, int c, int64_t voxels_per_sample,
                      float w_dice, float w_ce, float w_dice_img, float w_entropy, int softmax,
                      float* dlogits, fplx_stream_t stream);

/* ------------------------------------------------------------------ segmentation loss, second family
 * The seven remaining losses of the reference's SegLossDict (loss/loss_dict_seg.py:31-41) fused with the four terms above:
 * FocalDice (dice.py:147-161), NoiseRobustDice (dice.py:181-199), ExpLog (exp_log.py:29-56), GeneralizedCE (ce.py:68-93),
 * MAE / MSE (mse.py) and SLSR (slsr.py:34-58).  ONE forward pass over logits, label and pixel_weight makes the 6C + 3 sums of
 * the first family (same positions) and the new ones behind them; ONE backward pass writes dlogits for any mixture.  Tensors,
 * `softmax`, `part` (rows = fplx_loss_rows, K = FPLX_LOSS_EXT_K(C)), image_weight, gscale and the data-parallel split
 * (sums -> all-reduce of totals -> from_sums with n_global) are as above.
 *   cfg    HOST floats [FPLX_LOSS_EXT_NCFG(C)], read during the call (the caller may reuse the array at once):
 *            [0..3]   w_dice, w_ce, w_dice_img, w_entropy            the first family's term weights
 *            [4..10]  w_focal, w_noise_robust, w_explog, w_gce, w_mae, w_mse, w_slsr
 *            [11]     beta        FocalDiceLoss_beta
 *            [12]     gamma_nr    NoiseRobustDiceLoss_gamma
 *            [13]     w_dice_el   ExpLogLoss_w_dice
 *            [14]     gamma_el    ExpLogLoss_gamma
 *            [15]     q           loss_gce_q
 *            [16]     epsilon     slsrloss_epsilon
 *            [17]     use_pixel_weight (0 / 1)  GeneralizedCE weights by pixel_weight and divides by its sum (no epsilon);
 *                     pixel_weight must then be given (FPLX_E_NULL otherwise)
 *            [18..18+C-1]  GeneralizedCE class weights (all 1 for none)
 *          A term whose weight is 0 is not evaluated in the voxel loops.
 *   What pixel_weight means per term, as in the reference: Dice / CE / image-weighted Dice weight by it; FocalDice,
 *   NoiseRobustDice, ExpLog, MAE and MSE ignore it; SLSR reads it as a mask (> 0: the label is smoothed); GeneralizedCE uses
 *   it only with cfg[17].
 *   sums / totals: double [N][K] / [K], K = FPLX_LOSS_EXT_K(C): [0, 6C + 3) as FPLX_LOSS_K; then per class c four entries at
 *          6C + 3 + 4c: sum p, sum y p (both unweighted), sum |p - y|^gamma_nr, sum y (-log(0.005 + 0.99 p))^gamma_el; then at
 *          10C + 3: the GeneralizedCE numerator, sum (p - y)^2, sum |p - y|, the SLSR numerator.
 *   out    fp32 device [FPLX_LOSS_EXT_NOUT(C)]: [0] total of all eleven terms, [1..3] and [4, 4 + C) as above, then the values
 *          of FocalDice, NoiseRobustDice, ExpLog, GeneralizedCE, MAE, MSE, SLSR (unweighted).
 *   coef   fp32 device [FPLX_LOSS_EXT_NCOEF(N, C)] */
#define FPLX_LOSS_EXT_K(C) (10 * (C) + 7)
#define FPLX_LOSS_EXT_NCFG(C) (18 + (C))
#define FPLX_LOSS_EXT_NOUT(C) (4 + (C) + 7)
#define FPLX_LOSS_EXT_NCOEF(N, C) ((N) * (C) * 2 + 2 + 4 * (C) + 4)
int fplx_seg_loss_ext_fwd(const float* logits, const float* label, const float* pixel_weight, const float* image_weight,
                          int n, int c, int64_t voxels_per_sample, const float* cfg, int softmax, float* part, float* out,
                          float* coef, fplx_stream_t stream);
int fplx_seg_loss_ext_sums(const float* logits, const float* label, const float* pixel_weight, int n, int c,
                           int64_t voxels_per_sample, const float* cfg, int softmax, float* part, double* sums,
                           double* totals, fplx_stream_t stream);
int fplx_seg_loss_ext_from_sums(const double* sums, const double* totals, const float* image_weight, int n, int n_global,
                                int c, int64_t voxels_per_sample, int has_pixel_weight, const float* cfg, float* out,
                                float* coef, fplx_stream_t stream);
int fplx_seg_loss_ext_bwd(const float* logits, const float* label, const float* pixel_weight, const float* coef,
                          const float* gscale, int n, int c, int64_t voxels_per_sample, const float* cfg, int softmax,
                          float* dlogits, fplx_stream_t stream);

/* ------------------------------------------------------------------ optimiser
 * torch.optim.Adam(lr, weight_decay) as built by net_run_dsbn/get_optimizer.py:17 on a flat
 * fp32 buffer: g += wd*p; m,v moments; bias correction with `step` (1-based); p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps).
 * grad_scale multiplies g first (1/world_size after an all-reduce sum).  This is fplx_optim_step (below) with kind
 * FPLX_OPT_ADAM, s0 = m, s1 = v and hp = {lr, beta1, beta2, eps, weight_decay}: same kernel, same refusals. */
int fplx_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, float grad_scale, fplx_stream_t stream);
/* fplx_adam_step over the flat segment [0, n) AND, in the same launch, the bf16 packs fplx_pack_conv_weights_batched makes
 * of the `nl` (<= 32) 3x3x3 convolution weights that live inside it - from the UPDATED values (the weights change only here;
 * what the train step otherwise re-reads at the head of every forward, unet2d5_dsbn.py:54-55 + get_optimizer.py:17).
 * off[i]: element offset of layer i's [cout][cin][3][3][3] weight in the segment (ascending, multiples of 4); layers must
 * satisfy fplx_adam_pack_ok; wb[i] may be NULL; stamp: as in fplx_pack_conv_weights_batched (may be NULL), written from the
 * updated values.  p, g, m and v must be 16-byte aligned.  Same parameters, moments and packs as the two separate calls,
 * bit for bit.  This is fplx_optim_pack_step (below) with kind FPLX_OPT_ADAM, s0 = m, s1 = v and fplx_adam_step's hp. */
int fplx_adam_pack_ok(int cout, int cin);
int fplx_adam_pack_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float grad_scale, int nl, const int64_t* off, const int* cout,
                        const int* cin, void* const* wf, void* const* wb, float* const* stamp, fplx_stream_t stream);
/* Every optimiser get_optimizer can run (net_run_dsbn/get_optimizer.py:13-34; it passes lr, momentum and
 * weight_decay only, everything else is torch's default), one launch over a flat fp32 segment, with the arithmetic of torch's
 * _single_tensor_* functions.  p, g, s0, s1: any 4-byte-aligned base, any n > 0.  hp: HOST array of nhp floats; s0 / s1: the
 * kind's state streams, read and written (a stream the kind does not have is never touched and may be NULL):
 *   kind                hp                                               s0               s1
 *   FPLX_OPT_SGD        lr, momentum, weight_decay                       momentum_buffer  -               get_optimizer.py:13-15
 *                       (momentum == 0: no state at all; the first buffer is the gradient, i.e. momentum * 0 + g)
 *   FPLX_OPT_ADADELTA   lr, rho, eps, weight_decay                       square_avg       acc_delta       get_optimizer.py:20-21
 *   FPLX_OPT_ADAGRAD    lr, lr_decay, eps, weight_decay                  sum              -               get_optimizer.py:22-23
 *   FPLX_OPT_ADAMAX     lr, beta1, beta2, eps, weight_decay              exp_avg          exp_inf         get_optimizer.py:24-25
 *   FPLX_OPT_ASGD       eta, mu, lambd, weight_decay                     ax               -               get_optimizer.py:26-27
 *                       (eta and mu are the caller's per-segment scalars: torch forms the next step's pair after the update,
 *                        eta = lr / (1 + lambd lr step)^alpha, mu = 1 / max(1, step - t0); they start as lr and 1)
 *   FPLX_OPT_RMSPROP    lr, alpha, eps, momentum, weight_decay           square_avg       momentum_buffer get_optimizer.py:30-32
 *                       (s1 only if momentum > 0; not centred)
 *   FPLX_OPT_RPROP      lr, etaminus, etaplus, step_min, step_max        prev             step_size       get_optimizer.py:33-34
 *                       (no weight decay; at step == 1 the incoming s0 / s1 are ignored: prev = 0, step_size = lr)
 *   FPLX_OPT_ADAM       lr, beta1, beta2, eps, weight_decay              exp_avg          exp_avg_sq      get_optimizer.py:16-17
 * step (1-based) enters Adagrad's lr / (1 + (step - 1) lr_decay), Adamax's and Adam's lr / (1 - beta1^step) and Adam's
 * 1 / sqrt(1 - beta2^step), formed in double on the host and rounded once; grad_scale multiplies g first (for Rprop that keeps
 * sign and zero, which is all it reads).
 * FPLX_E_BADSHAPE: unknown kind, n <= 0, step < 1, wrong nhp; FPLX_E_NULL: a missing pointer the kind needs. */
enum { FPLX_OPT_SGD = 0, FPLX_OPT_ADADELTA, FPLX_OPT_ADAGRAD, FPLX_OPT_ADAMAX, FPLX_OPT_ASGD, FPLX_OPT_RMSPROP, FPLX_OPT_RPROP,
       FPLX_OPT_ADAM, FPLX_OPT_COUNT };
int fplx_optim_step(int kind, float* p, const float* g, float* s0, float* s1, int64_t n, const float* hp, int nhp, int step,
                    float grad_scale, fplx_stream_t stream);
/* fplx_optim_step AND the bf16 packs of the 3x3x3 weights inside the segment in one launch: nl, off, cout, cin, wf, wb and
 * stamp as fplx_adam_pack_step describes them (layer rule: fplx_adam_pack_ok); p, g and the kind's state streams must be
 * 16-byte aligned.  Same parameters, state and packs as fplx_optim_step followed by fplx_pack_conv_weights_batched, bit for
 * bit. */
int fplx_optim_pack_step(int kind, float* p, const float* g, float* s0, float* s1, int64_t n, const float* hp, int nhp, int step,
                         float grad_scale, int nl, const int64_t* off, const int* cout, const int* cin, void* const* wf,
                         void* const* wb, float* const* stamp, fplx_stream_t stream);

/* ------------------------------------------------------------------ pseudo-label filter
 * FPL branch of SegmentationAgent.infer (net_run_dsbn/agent_seg.py:911-931) for one volume:
 * logits fp32 [T][C][V] (T MC/TTA passes; 1 <= T <= 16 and 2 <= C <= 4, anything else is refused with FPLX_E_BADSHAPE).
 * Per voxel: softmax per pass (scipy.special.softmax,
 * fp32), hard label per pass (argmax, uint8 [T][V], may be NULL), population variance over T
 * summed over classes, mean_T p_1, u = -m*log(m+1e-6), boundary = #(u > thr).
 *   part  workspace fp32/int [rows][2] (rows = fplx_num_partials(V))
 *   out   device double [4]: vars, boundary, uncer_one (= 1 if boundary < 50 else vars/boundary), 0
 *   mean_out / unc_out optional fp32 [V] maps */
int fplx_mc_filter(const float* logits, int t, int c, int64_t v, float thr, uint8_t* hards,
                   float* mean_out, float* unc_out, double* part, double* out, fplx_stream_t stream);
/* save_outputs (agent_seg.py:1049-1050): softmax -> argmax -> uint8.  logits fp32 [N][C][V] */
int fplx_hard_label(const float* logits, int n, int c, int64_t v, uint8_t* out, fplx_stream_t stream);
/* data/get_pixel_weight.py:21-26 (/root/reference): w = 1 - 0.5*xor(a,b) (a,b uint8 {0,1}) as fp32
 * (exact in fp32: values are 1.0 / 0.5), followed, if apply_set_weight, by
 * NiftyDataset.set_weight_ (io/nifty_dataset.py:165-168): w<1 -> 0, w *= image_weight. */
int fplx_pixel_weight(const uint8_t* a, const uint8_t* b, int64_t v, int apply_set_weight, float image_weight,
                      float* out, fplx_stream_t stream);

/* ------------------------------------------------------------------ training-sample transforms
 * The reference's numpy chain train_transform = [NormalizeWithMeanStd, Pad, RandomCrop, RandomFlip,
 * LabelToProbability] (config_dual/data_vs/vs_t1s_g.cfg:21) on device volumes [C][D][H][W]; the random draws stay on
 * the host (fplx/transform.py, Python `random` in the reference's order).
 *  normalize: y = (x - mean) / std per call (one channel); mean_std == NULL -> float32 mean / population std of x
 *             (PyMIC/pymic/transform/normalize.py:43-68); ws of fplx_normalize_ws_bytes() bytes; out_mean_std may be NULL
 *  normalize_positive: NormalizeWithMeanStd_ignore_non_positive (normalize.py:55-66): mean / std over the voxels > 0, y =
 *             (x - mean) / std there and noise[i] elsewhere (noise: the caller's numpy.random.normal(0, 1) draw, as fp32);
 *             y may alias x
 *  pad_reflect: numpy.pad(mode='reflect') with lower margins lo_* (pad.py:126-163); elem_bytes 4 (fp32) or 1 (uint8)
 *  crop_flip: crop box [c*, c*+o*) then flip of the cropped patch, flip_mask bit0 = W, bit1 = H, bit2 = D
 *             (crop.py:27-49, flip.py:34-62)
 *  label_bbox: out9 = [count, min c,d,h,w, max+1 c,d,h,w] of {label in mask_labels} (util/image_process.py:8-34)
 *  label_to_probability: one-hot fp32 [class_num][voxels] (label_convert.py:82-94)
 *  set_weight: in place pw = (pw < 1 ? 0 : pw) * image_weight (PyMIC/pymic/io/nifty_dataset.py:165-168) */
size_t fplx_normalize_ws_bytes(void);
int fplx_normalize_mean_std(const float* x, float* y, int64_t n, const float* mean_std, void* ws, size_t ws_bytes,
                            float* out_mean_std, fplx_stream_t stream);
int fplx_normalize_positive(const float* x, const float* noise, float* y, int64_t n, void* ws, size_t ws_bytes,
                            float* out_mean_std, fplx_stream_t stream);
int fplx_pad_reflect(const void* x, void* y, int elem_bytes, int c, int d, int h, int w, int lo_d, int lo_h, int lo_w,
                     int od, int oh, int ow, fplx_stream_t stream);
int fplx_crop_flip(const void* x, void* y, int elem_bytes, int c, int d, int h, int w, int cd, int ch, int cw, int od,
                   int oh, int ow, int flip_mask, fplx_stream_t stream);
int fplx_label_bbox(const unsigned char* label, int c, int d, int h, int w, const int* mask_labels, int nmask, int* out9,
                    fplx_stream_t stream);
int fplx_label_to_probability(const unsigned char* label, float* prob, int class_num, int64_t voxels,
                              fplx_stream_t stream);
int fplx_set_weight(float* pixel_weight, int64_t n, float image_weight, fplx_stream_t stream);

/* ------------------------------------------------------------------ crop, bounding-box and label transforms (csrc/crop_label.hip)
 * CenterCrop / CropWithBoundingBox and their inverse, LabelConvert / LabelConvertNonzero, PartialLabelToProbability
 * (PyMIC/pymic/transform/crop.py:13-167, label_convert.py:27-130).  The forward crops gather with fplx_crop_flip.
 *  nonzero_bbox: out9 = [count, min c,d,h,w, max+1 c,d,h,w] (the layout of fplx_label_bbox) of {x != 0} over a fp32 volume
 *             [c][d][h][w], numpy.nonzero's test: every bit pattern but +0.0 and -0.0 counts (a NaN does, -0.0 does not).
 *             Integer min / max / sum only: the result does not depend on the order of the blocks.  count == 0 leaves
 *             min = INT_MAX, max = 0.  Fewer than 2^31 elements.
 *  label_lut: out[i] = lut256[in[i]] (lut256: 256 bytes in DEVICE memory); out may be in.  The host builds the table with
 *             convert_label's arithmetic (util/image_process.py:194-208): the sum of the targets of every matching source,
 *             mod 256; labels that are not listed map to 0.
 *  partial_label_to_probability: prob[k][v] = (label[v] == k) for k < class_num, weight[v] = 1 - (label[v] == class_num),
 *             *max_label (device int) = the largest label (label_convert.py:122-130; the caller raises when it exceeds
 *             class_num).
 *  paste_roi: out [c][od][oh][ow] = 0 outside the box [lo, lo + s), sub [c][sd][sh][sw] inside: numpy.zeros +
 *             set_ND_volume_roi_with_bounding_box_range (crop.py:83-108) with every element written exactly once;
 *             elem_bytes 4 or 1; sub and out must not overlap.
 * Refused before any launch: FPLX_E_NULL, FPLX_E_BADSHAPE (non-positive extent, box outside the output, class_num outside
 * 1..255), FPLX_E_BADDTYPE (element size). */
int fplx_nonzero_bbox(const float* x, int c, int d, int h, int w, int* out9, fplx_stream_t stream);
int fplx_label_lut(const uint8_t* in, uint8_t* out, int64_t n, const uint8_t* lut256, fplx_stream_t stream);
int fplx_partial_label_to_probability(const uint8_t* label, float* prob, float* weight, int class_num, int64_t voxels,
                                      int* max_label, fplx_stream_t stream);
int fplx_paste_roi(const void* sub, void* out, int elem_bytes, int c, int sd, int sh, int sw, int od, int oh, int ow,
                   int lo_d, int lo_h, int lo_w, fplx_stream_t stream);

/* ------------------------------------------------------------------ geometric augmentation: affine resampling
 * RandomRotate / Rescale / RandomRescale (PyMIC/pymic/transform/rotate.py:14-92, rescale.py:14-153), which the reference
 * runs as scipy.ndimage.rotate / scipy.ndimage.zoom on the host.  y[ch][o] = interp(x[ch], M o + t) for x [c][d][h][w]
 * and y [c][od][oh][ow], o = (o_d, o_h, o_w), with scipy's semantics for mode='constant', cval=0:
 *  coordinates fp64, c_i = ((o_0 M[i][0] + o_1 M[i][1]) + o_2 M[i][2]) + t_i (offset last, no fused multiply-add);
 *  any c_i < 0 or c_i > n_i - 1 (or NaN) -> 0;  order 0: x[floor(c_i + 0.5)];  order 1: weights (1 - y, 1 - (1 - y)) with
 *  y = c - floor(c), fp64 sum over the 8 neighbours of ((x * w_d) * w_h) * w_w, k_d outermost, one cast to fp32.
 *  elem_bytes 4 (fp32, order 0 or 1) or 1 (uint8, order 0 only); matrix9 (row-major 3x3) and offset3 are HOST arrays of
 *  doubles, read before the call returns and passed to the kernel by value; one launch covers all channels; x and y
 *  must not overlap.
 * Refused before any launch: FPLX_E_NULL for a missing pointer; FPLX_E_BADSHAPE for a non-positive extent, 2^31 elements
 * or more on either side, or an order other than 0 / 1; FPLX_E_BADDTYPE for another element size or uint8 with order 1. */
int fplx_resample_affine(const void* x, void* y, int elem_bytes, int order, int c, int d, int h, int w, int od, int oh,
                         int ow, const double* matrix9, const double* offset3, fplx_stream_t stream);

/* ------------------------------------------------------------------ dataset preparation: cubic-spline resampling
 * scipy.ndimage.zoom / rotate / affine_transform at their default spline order 3, which the reference's preparation uses
 * (data/preprocess_vs.py:107-135: ndimage.zoom(img_sub, zoom); PyMIC/pymic/util/image_process.py:210-228: any order).
 * Two steps, as in scipy; fplx.ops.resample_spline runs both.
 *
 * fplx_spline_prefilter: x [c][d][h][w] fp32 -> coef [c][d][h][w] fp64, the B-spline coefficients under scipy's mirror
 *  boundary: the recursive filter with pole z = sqrt(3) - 2 along every line of D, then H, then W.  Per line of length
 *  n > 1: c *= (1 - z)(1 - 1/z);  c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} z^i (c[i] + z^(n-1) c[n-1-i])) /
 *  (1 - z^(2n-2));  c[i] += z c[i-1];  c[n-1] = (z c[n-2] + c[n-1]) z / (z z - 1);  c[i] = z (c[i+1] - c[i]) downwards; a
 *  line of length 1 is left alone.  All sums run in that one order, without atomics: bitwise reproducible.  x and coef
 *  must not overlap.
 * fplx_resample_spline: y[ch][o] = sum over the 4x4x4 taps of coef * w_d * w_h * w_w at M o + t in fp64, one cast to fp32;
 *  coordinates and the outside rule (c_i < 0, c_i > n_i - 1 or NaN -> 0) are fplx_resample_affine's; taps floor(c) - 1 + k,
 *  k = 0..3, reflected about the first and last sample (period 2n - 2; an axis of extent 1 reads index 0); weights with
 *  y = c - floor(c), zc = 1 - y: w1 = (y y (y - 2) 3 + 4) / 6, w2 = (zc zc (zc - 2) 3 + 4) / 6, w0 = zc zc zc / 6,
 *  w3 = 1 - w0 - w1 - w2; the value is multiplied by one axis weight after the other, k_d outermost, k_w innermost.
 *  matrix9 and offset3 are HOST arrays of doubles, read before the call returns; coef and y must not overlap.
 * Refused before any launch: FPLX_E_NULL for a missing pointer; FPLX_E_BADSHAPE for a non-positive extent, 2^31 elements or
 * more on either side, or an order other than 3 (orders 2, 4 and 5 are not built; the message names the built order). */
int fplx_spline_prefilter(const float* x, double* coef, int c, int d, int h, int w, int order, fplx_stream_t stream);
int fplx_resample_spline(const double* coef, float* y, int c, int d, int h, int w, int od, int oh, int ow,
                         const double* matrix9, const double* offset3, int order, fplx_stream_t stream);

/* ------------------------------------------------------------------ exact Euclidean distance transform
 * scipy.ndimage.distance_transform_edt, which get_euclidean_distance calls on image > 0.5 and on image <= 0.5
 * (PyMIC/pymic/util/image_process.py:165-192); fplx.image_process mirrors both.
 *
 * fplx_edt_squared: mask uint8 [n][d][h][w] (nonzero = foreground; ndim = 2: a 2D mask, d must be 1) -> sq fp64 [n][d][h][w],
 *  the SQUARED distance of every voxel to the nearest background voxel of its mask under the sampling (sz, sy, sx)
 *  (sampling3: HOST array of 3 doubles, read before the call returns; ndim = 2 uses sampling3[1] and [2] only; all three must be valid): with g0 = 0 on
 *  background and +inf on foreground, for axis 0, then 1, then 2: g[j] = min_i (g[i] + ((j - i) s_axis)^2) - product, square,
 *  sum, each rounded to fp64, none contracted - which equals scipy's min over the background of
 *  ((dz sz)^2 + (dy sy)^2) + (dx sx)^2 bit for bit.  Background voxels get exactly 0.  No atomics: bitwise reproducible.
 *  phantom: device uint8 [n] or NULL; phantom[m] != 0 states that mask m has NO background voxel (the caller's reduction):
 *  the result is then scipy's, the distance to one background voxel at index (-1, 0, 0) (2D: (-1, 0)).  A mask without
 *  background whose flag is not set yields +inf everywhere.
 *  idx: NULL, or int32 [n][ndim][d][h][w], the feature transform: the coordinates (z, y, x) (2D: (y, x)) of a background voxel
 *  at that distance ((-1, 0, 0) under phantom); among several at the same distance scipy may name another.  It needs
 *  ws: int32 workspace of at least FPLX_EDT_WS_BYTES(n, d * h * w) bytes (unused and may be NULL when idx is NULL).
 * fplx_edt_pass: ONE of those passes alone, in place on a fp64 map g [n][d][h][w] along axis 0 (d), 1 (h) or 2 (w) with the
 *  sampling of that axis: g[j] = min_i (g[i] + ((j - i) s)^2) on every line; +inf entries are allowed, a line without a
 *  finite entry stays +inf.  The three calls on g0 reproduce fplx_edt_squared for a mask with background; the benchmark
 *  (tools/edt_bench.py) times the passes with it.
 * fplx_edt_finish: out[i] = sqrt(sq_a[i]) when sq_b is NULL, else sqrt(sq_b[i]) - sqrt(sq_a[i]) (the signed map of
 *  get_euclidean_distance: a = image > 0.5, b = image <= 0.5, both from ONE fplx_edt_squared call with n = 2), i < count;
 *  out must not overlap the inputs.
 * Refused before any launch: FPLX_E_NULL for a missing pointer; FPLX_E_BADSHAPE for a non-positive extent, an extent above
 * FPLX_EDT_MAX_EXTENT (a block stages whole lines in LDS; the message names the limit), 2^31 elements or more, ndim other than
 * 2 or 3, an axis other than 0..2, or a sampling that is not positive and finite; FPLX_E_WORKSPACE for a workspace that is too small. */
#define FPLX_EDT_MAX_EXTENT 620
#define FPLX_EDT_WS_BYTES(n, voxels) ((size_t)2 * (size_t)(n) * (size_t)(voxels) * 4)
int fplx_edt_squared(const uint8_t* mask, int n, int d, int h, int w, int ndim, const double* sampling3, const uint8_t* phantom,
                     double* sq, int* idx, int* ws, size_t ws_bytes, fplx_stream_t stream);
int fplx_edt_pass(double* g, int n, int d, int h, int w, int axis, double sampling, fplx_stream_t stream);
int fplx_edt_finish(const double* sq_a, const double* sq_b, double* out, int64_t count, fplx_stream_t stream);

/* ------------------------------------------------------------------ Inferer: sliding window + flip TTA
 * PyMIC/pymic/net_run_dsbn/infer_func.py:50-112 (tiling, overlap averaging), 188-222 (tta_mode 1).
 * The tile grid is the Cartesian product of per-axis start lists (HOST arrays, at most 64 entries each, non-decreasing,
 * first 0, last start + window == size; a clamped duplicate start is a separate tile, as in the reference's list);
 * tile index = (iw * nh + ih) * nd + id, the reference's enumeration order.  flips: HOST array of 1..4 masks,
 * bit0 = W axis flipped, bit1 = H axis flipped (reference order: 0, 2, 1, 3).
 *  fplx_sw_extract: image fp32 [n][c][d][h][w] -> patches [nflips][tiles][n][c][wd][wh][ww]: tile t of flip f is cut from
 *                   the flipped image.
 *  fplx_sw_merge:   predictions [nflips][tiles][n][c][wd][wh][ww] (c = classes) -> out [n][c][d][h][w]: per flip the
 *                   sum over the covering tiles IN TILE ORDER divided by their number (no division when there is one
 *                   tile), flipped back, then ((o1 + o2) + o3 + o4) / nflips - the reference's additions in its order.
 *  fplx_sw_merge_mc: the same for `passes` Monte-Carlo predictions of every patch in ONE launch (agent_seg.py:898-909 calls
 *                   the inferer once per pass) -> out [passes][n][c][d][h][w], reading the predictions where the network wrote
 *                   them: it ran on chunks of `chunk` consecutive patches (the last one shorter) and each call produced all
 *                   passes of its chunk, pass-major - [chunks][passes][patches of the chunk][c][wd][wh][ww].
 *                   fplx_sw_merge == passes 1, chunk = all patches. */
int fplx_sw_extract(const float* image, int n, int c, int d, int h, int w, const int* starts_d, int nd, const int* starts_h,
                    int nh, const int* starts_w, int nw, int wd, int wh, int ww, const int* flips, int nflips, float* patches,
                    fplx_stream_t stream);
int fplx_sw_merge(const float* patches, int n, int c, int d, int h, int w, const int* starts_d, int nd, const int* starts_h,
                  int nh, const int* starts_w, int nw, int wd, int wh, int ww, const int* flips, int nflips, float* out,
                  fplx_stream_t stream);
int fplx_sw_merge_mc(const float* patches, int passes, int chunk, int n, int c, int d, int h, int w, const int* starts_d, int nd,
                     const int* starts_h, int nh, const int* starts_w, int nw, int wd, int wh, int ww, const int* flips,
                     int nflips, float* out, fplx_stream_t stream);

/* ------------------------------------------------------------------ evaluation
 * Exact voxel counts behind binary_dice / binary_iou / rve / volume (PyMIC/pymic/util/evaluation_seg_train.py:21-50,
 * 68-81, 171-186, 220-225): out[row][3] = {|seg==l & gt==l|, |seg==l|, |gt==l|} (uint64) for each of the nlabels labels
 * (<= 16), or ONE row counting membership in the label list when fuse != 0 (get_multi_class_evaluation_score, 231-262).
 * The scores themselves are float64 host arithmetic on these integers (fplx/evaluation.py). */
int fplx_overlap_counts(const unsigned char* seg, const unsigned char* gt, int64_t n, const int* labels, int nlabels,
                        int fuse, unsigned long long* out, fplx_stream_t stream);

/* Surface metrics behind binary_assd / binary_hd95 (PyMIC/pymic/util/evaluation_seg_train.py:84-99, 101-135, 137-171).
 * fplx_surface_edge_points: get_edge_points - edge = img - binary_erosion(img, cross) of a binary [d][h][w] volume (d = 1: the
 * 2D form, no depth neighbours); outside the volume is background.
 * fplx_surface_min_dist replaces the reference's GeodisTK.geodesic3d_raster_scan(zeros, seeds, spacing, 0.0, 2) (a
 * third-party C++ extension the reference imports, version unpinned, absent here) sampled at the query voxels:
 * out[i] = length of the shortest 26-neighbour lattice path from query i to the nearest seed with Euclidean step
 * lengths under spacing (sz, sy, sx) - the fixed point of that raster scan on a constant image; 1e10 when ns = 0.
 * Coordinates are int32 (z, y, x) triples.  PARITY UNPINNED against GeodisTK itself (see oracle/np_ref.py ev_raster_scan). */
int fplx_surface_edge_points(const unsigned char* img, int d, int h, int w, unsigned char* edge, fplx_stream_t stream);
int fplx_surface_min_dist(const int* query_zyx, int64_t nq, const int* seed_zyx, int64_t ns, float sz, float sy, float sx,
                          float* out, fplx_stream_t stream);

/* ------------------------------------------------------------------ prediction post-processing
 * Connected components of a uint8 volume seg [d][h][w] (d = 1: the 2D form), d * h * w < 2^31, under the 6-face
 * connectivity of scipy.ndimage.generate_binary_structure(3, 1) (4 neighbours in 2D).  Two neighbours join when
 * per_class == 0: both values are nonzero; per_class != 0: both values are equal and nonzero (every class in one pass).
 *  fplx_cc_label: labels int32 [d][h][w] = the C-order linear index of the first voxel of the voxel's component (canonical
 *                 labels), -1 for background.  Replaces scipy.ndimage.label in get_largest_k_components
 *                 (PyMIC/pymic/util/image_process.py:139-163).
 *  fplx_keep_largest_component: out uint8 [d][h][w] = seg where the voxel's component has the largest size among the
 *                 components of its class (per_class == 0: one class, all foreground), else 0; every component of the
 *                 maximal size is kept.  PostKeepLargestComponent (PyMIC/pymic/util/post_process.py:19-49), called by
 *                 save_outputs (net_run_dsbn/agent_seg.py:1052-1054) - mode 1: per_class = 0, mode 2: per_class = 1.
 *  ws: int32 workspace of at least FPLX_CC_LABEL_WS_BYTES / FPLX_KLC_WS_BYTES(d * h * w) bytes; ws[0] is the error word: 0
 *      after a good run, nonzero when a union-find loop reached its iteration cap (the result is then invalid) - the
 *      caller reads it after the stream has run the launches.
 * Both return FPLX_E_NULL / FPLX_E_BADSHAPE / FPLX_E_WORKSPACE before any launch for a missing pointer or workspace, a
 * non-positive dimension, 2^31 voxels or more, or a workspace that is too small. */
#define FPLX_CC_LABEL_WS_BYTES(voxels) ((size_t)320 * 4)
#define FPLX_KLC_WS_BYTES(voxels) (((size_t)320 + 2 * (size_t)(voxels)) * 4)
int fplx_cc_label(const uint8_t* seg, int d, int h, int w, int per_class, int* labels, int* ws, size_t ws_bytes,
                  fplx_stream_t stream);
int fplx_keep_largest_component(const uint8_t* seg, int d, int h, int w, int per_class, uint8_t* out, int* ws,
                                size_t ws_bytes, fplx_stream_t stream);

/* ------------------------------------------------------------------ intensity transforms
 * NormalizeWithMinMax / NormalizeWithPercentiles (PyMIC/pymic/transform/normalize.py:155-237), ChannelWiseThreshold /
 * ChannelWiseThresholdWithNormalize (threshold.py:14-132), GammaCorrection / GaussianNoise (intensity.py:14-86) on ONE channel
 * volume x of n fp32 voxels, 0 < n < 2^31; y may alias x in every element pass.  All fp32 arithmetic is numpy's on a float32
 * array under NumPy 2, operation for operation and without fused multiply-add; comparisons are written as numpy's masks
 * (x < v0 -> v0), so a NaN voxel passes through a clip.
 *  channel_minmax: out4 (device) = {min, max, min, max of the clipped data}, clipped = x < lo -> lo (if use_lo), then
 *             x > hi -> hi (if use_hi).  Any NaN voxel makes all four NaN, as numpy's min / max do.  ws: 16 bytes.
 *  select_kth: exact order statistics by radix selection (4 passes of 8 bits over an order-preserving integer key, no sort,
 *             no host round trip, integer arithmetic only).  ranks: HOST array of 1..4 ranks k_j in [0, n), read before the
 *             call returns; out (device) [nranks][2] = {s[k_j], s[min(k_j + 1, n - 1)]} of the ascending order s in which
 *             NaNs come last, as in numpy's sort.  -0.0 and +0.0 are equal values and either may be returned for a tie
 *             between them.  ws of fplx_select_ws_bytes() bytes.  A rank outside [0, n): FPLX_E_BADSHAPE before any launch.
 *  clip_affine: y = (clip(x, v0, v1) - a) / b with clip as above; _dev reads v0, v1, a and hi from device memory and uses
 *             b = *hi - *a (fp32), so a reduction feeds the pass without a host synchronisation.
 *  threshold_replace: x < t_lo -> r_lo (if use_lo), then the result > t_hi -> r_hi (if use_hi).
 *  normalize_range: ChannelWiseThresholdWithNormalize, mean_std_mode: float32 mean / population std over the voxels with
 *             v0 < x < v1 (each bound optional; fp64 accumulation), y = (x - mean) / std there and noise[i] elsewhere (a NaN
 *             voxel is elsewhere); an empty mask gives NaN moments and y = noise.  ws of fplx_normalize_ws_bytes() bytes;
 *             out_mean_std may be NULL.
 *  gamma:     d = *vmax - *vmin (device scalars); y = float32(pow(double((x - *vmin) / d), double(gamma))) * d + *vmin.
 *  add_noise_f64: y = float32(double(x) + noise[i]) for the caller's fp64 noise volume (numpy.random.normal on the host).
 *  add_noise_philox (no reference counterpart): element i takes words 2 (i & 1) and 2 (i & 1) + 1 of Philox4x32-10 with
 *             counter (i >> 1, 0, stream_id, 0) and key (seed low, seed high); u = (word + 1) / 2^32 in (0, 1];
 *             z = sqrt(-2 ln u1) cos(2 pi u2) in fp64; y = float32((double(x) + mean) + sigma * z).  out_uniforms (may be
 *             NULL): fp64 [n][2] = {u1, u2}. */
int fplx_channel_minmax(const float* x, int64_t n, float lo, int use_lo, float hi, int use_hi, void* ws, size_t ws_bytes,
                        float* out4, fplx_stream_t stream);
size_t fplx_select_ws_bytes(void);
int fplx_select_kth(const float* x, int64_t n, const int64_t* ranks, int nranks, float* out, void* ws, size_t ws_bytes,
                    fplx_stream_t stream);
int fplx_clip_affine(const float* x, float* y, int64_t n, float v0, float v1, float a, float b, fplx_stream_t stream);
int fplx_clip_affine_dev(const float* x, float* y, int64_t n, const float* v0, const float* v1, const float* a,
                         const float* hi, fplx_stream_t stream);
int fplx_threshold_replace(const float* x, float* y, int64_t n, float t_lo, float r_lo, int use_lo, float t_hi, float r_hi,
                           int use_hi, fplx_stream_t stream);
int fplx_normalize_range(const float* x, const float* noise, float* y, int64_t n, float v0, int use_v0, float v1, int use_v1,
                         void* ws, size_t ws_bytes, float* out_mean_std, fplx_stream_t stream);
int fplx_gamma(const float* x, float* y, int64_t n, const float* vmin, const float* vmax, float gamma, fplx_stream_t stream);
int fplx_add_noise_f64(const float* x, const double* noise, float* y, int64_t n, fplx_stream_t stream);
int fplx_add_noise_philox(const float* x, float* y, int64_t n, uint64_t seed, uint32_t stream_id, double mean, double sigma,
                          double* out_uniforms, fplx_stream_t stream);

/* ------------------------------------------------------------------ semi-supervised learning (csrc/ssl.hip)
 * What the reference's second entry point adds to an iteration (PyMIC/pymic/net_run_ssl/ssl_em.py, ssl_mt.py, ssl_uamt.py),
 * each as one pass.  Logits fp32 [N][C][V] contiguous, 2 <= C <= 8, 1 <= N <= 65535, any V >= 1.  Reductions as in the loss
 * families: `part` fp32 [N][fplx_loss_rows(V)][K] (the block partials; K = 2 for the consistency, 1 for the entropy), the rows
 * summed in double in a fixed order - no floating-point atomics, two runs give the same bits.  A lane takes four voxels with
 * 16-byte loads where every tensor base is 16-byte aligned and V is a multiple of 4, else one voxel; the flat passes take
 * n / 4 quads and a scalar tail.  FPLX_E_BADSHAPE / FPLX_E_NULL before any launch.
 *  ssl_perturb: y[r][i] = x[i] + clamp(sigma z[r][i], -clip, clip), r < reps (1..64): `x1 + torch.clamp(torch.randn_like(x1) *
 *             0.1, -0.2, 0.2)` of ssl_mt.py:79 and, with reps = 2, ssl_uamt.py:83-85.  Three fp32 operations, none contracted:
 *             with z = the caller's fp32 noise[reps][n] the result is torch's on the CPU bit for bit.  noise NULL: z is drawn on the
 *             device - element i of repetition r takes words 2 (i & 1), 2 (i & 1) + 1 of Philox4x32-10 with counter
 *             (i >> 1, r, stream_id, i >> 33) and key (seed low, seed high), u = (word + 1) / 2^32, z = float32(sqrt(-2 ln u1)
 *             cos(2 pi u2)) formed in fp64 (the Box-Muller of add_noise_philox).
 *  ssl_consistency_fwd: student, teacher [N][C][V]; mc [T][N][C][V] or NULL with t = 0; t even, at most 16.  softmax = 1:
 *             softmax over C of all three inputs; 0: they are probabilities.  t = 0 (MeanTeacher) keeps every voxel; t > 0 (UAMT,
 *             ssl_uamt.py:91-99): m_c = (sum_t softmax(mc_t)_c) / T, unc = -sum_c m_c log(m_c + 1e-6), kept iff unc < thr,
 *             the flag written to mask uint8 [N][V] (needed iff t > 0).
 *             out double [4]: sum over kept voxels and classes of (p_c - q_c)^2; number of kept voxels; the loss; 0.
 *             loss = out0 / (N C V) for t = 0 (torch.nn.MSELoss(), ssl_mt.py:100), out0 / (2 out1 + 1e-16) for t > 0
 *             (ssl_uamt.py:100 - the 2 is the reference's literal, not C).
 *  ssl_consistency_bwd: e_c = 2 (p_c - q_c) k / D, k the kept flag (1 with t = 0), D the denominator above (read from out[1]
 *             on the device when t > 0; out may be NULL with t = 0); dstudent_c = gscale[0] p_c (e_c - sum_j p_j e_j), with
 *             softmax = 0 gscale[0] e_c.  gscale: device fp32 scalar.  The teacher receives no gradient.
 *  ssl_entropy_fwd / _bwd: EntropyLoss (loss/seg/ssl.py:32-44): p' = 0.999 p + 5e-4, H = -sum_c p'_c ln p'_c / ln C, loss = mean
 *             of H over N V.  out double [4]: sum over the voxels of -sum_c p'_c ln p'_c; N V; the loss; 0.  Backward:
 *             dL/dp_c = -0.999 (ln p'_c + 1) / (ln C N V), then the softmax Jacobian (softmax = 0: as it is), times gscale[0].
 *             (Not the first family's entropy term: that one is log2 with + 1e-10, agent_seg.py:352-354.)
 *  ema_step:  ema = alpha ema + (1 - alpha) p over a flat fp32 segment, 0 <= alpha <= 1 (`ema_param.data.mul_(alpha).add_(1 -
 *             alpha, param.data)`, ssl_mt.py:112-113, for all parameters in one launch); 1 - alpha is formed in double on the
 *             host and rounded once, the element is fma(alpha, ema, (1 - alpha) p).
 *  ssl_pyramid_fwd: URPC's regulariser (ssl_urpc.py:76-91) over K = 2..4 logit tensors given as a table of K device pointers,
 *             each [N][C][V], N counting the unlabelled rows only.  Per voxel p_k = softmax(z_k), m = (p_1 + .. + p_K) / K,
 *             a = 0.99 m + 0.005, q_k = 0.99 p_k + 0.005, var_k = sum_c a_c (ln a_c - ln q_kc), e_k = exp(-var_k),
 *             s_k = sum_c (a_c - q_kc)^2.  part fp32 [N][fplx_loss_rows(V)][3 K].  With M = N V:
 *             out double [K][4] + [2]: per scale A_k = sum s_k e_k, B_k = sum e_k, V_k = sum var_k,
 *             L_k = (A_k / (C M)) / (B_k / M + 1e-8) + V_k / M; then loss_reg = (sum_k L_k) / K and 0.
 *             The vector path takes four voxels per lane while K C <= 12, two beyond (K C values are live per voxel).
 *  ssl_pyramid_bwd: one launch writes the K tensors dlogits_j = gscale[0] d loss_reg / d z_j.  With A_k, B_k read from `out` on
 *             the device: alpha_k = 1 / (C M (B_k / M + 1e-8)), beta_k = -(A_k / (C M)) / (B_k / M + 1e-8)^2 / M,
 *             g_k = 1 / M - e_k (alpha_k s_k + beta_k), h_k = alpha_k e_k,
 *             dL/dp_jc = (0.99 / K) [(1 / K) sum_k (g_k (ln a_c - ln q_kc + 1) + 2 h_k (a_c - q_kc)) - g_j a_c / q_jc
 *             - 2 h_j (a_c - q_jc)] (the mean m carries gradient, as in the reference), then the softmax Jacobian.
 *  ssl_pseudo_onehot: K = 1..3 logit tensors (a pointer table) -> K fp32 one-hot tensors [N][C][V] of the FIRST maximum of the
 *             logits over C: `get_soft_label(argmax(softmax(z)))` of ssl_cps.py:103-106 in one launch, except that two
 *             distinct logits which fp32 softmax rounds to one probability keep their order here. */
int fplx_ssl_perturb(const float* x, const float* noise, float* y, int64_t n, int reps, float sigma, float clip, uint64_t seed,
                     uint32_t stream_id, fplx_stream_t stream);
int fplx_ssl_consistency_fwd(const float* student, const float* teacher, const float* mc, int t, int n, int c,
                             int64_t voxels_per_sample, float thr, int softmax, uint8_t* mask, float* part, double* out,
                             fplx_stream_t stream);
int fplx_ssl_consistency_bwd(const float* student, const float* teacher, const uint8_t* mask, const double* out,
                             const float* gscale, int n, int c, int64_t voxels_per_sample, int t, int softmax, float* dstudent,
                             fplx_stream_t stream);
int fplx_ssl_entropy_fwd(const float* logits, int n, int c, int64_t voxels_per_sample, int softmax, float* part, double* out,
                         fplx_stream_t stream);
int fplx_ssl_entropy_bwd(const float* logits, const float* gscale, int n, int c, int64_t voxels_per_sample, int softmax,
                         float* dlogits, fplx_stream_t stream);
int fplx_ema_step(float* ema, const float* p, int64_t n, float alpha, fplx_stream_t stream);
int fplx_ssl_pyramid_fwd(const float* const* logits, int k, int n, int c, int64_t voxels_per_sample, float* part, double* out,
                         fplx_stream_t stream);
int fplx_ssl_pyramid_bwd(const float* const* logits, const double* out, const float* gscale, int k, int n, int c,
                         int64_t voxels_per_sample, float* const* dlogits, fplx_stream_t stream);
int fplx_ssl_pseudo_onehot(const float* const* logits, int k, int n, int c, int64_t voxels_per_sample, float* const* onehot,
                           fplx_stream_t stream);

/* ------------------------------------------------------------------ weakly-supervised learning (csrc/wsl.hip)
 * The regularisers of the reference's third entry point (PyMIC/pymic/net_run_wsl/; loss/seg/gatedcrf.py, loss/seg/ssl.py:46-86
 * TotalVariationLoss, loss/seg/mumford_shah.py).  Logits fp32 [N][C][D][H][W] contiguous, 2 <= C <= 8; the image fp32
 * [N][Ci][D][H][W], 1 <= Ci <= 4; a slice is one (n, d) plane and the kernels index the 5-D tensors directly (the reference
 * transposes and copies to [N D][C][H][W]).  softmax = 1: softmax over C inside the kernel; 0: the input holds probabilities.
 * Reductions: fp32 block partials in `part`, summed in double in a fixed order by one wave - no floating-point atomics, two
 * runs give the same bits (the integer atomics on TV's count tensor commute).  out: double [4] on the device.  gscale: device
 * fp32 scalar.  dlogits_c = gscale[0] p_c (e_c - sum_j p_j e_j) with e = dLoss/dp (softmax = 0: gscale[0] e_c).
 * Limits: D H W <= 2^30, N C <= 65535, N D <= 65535.  FPLX_E_BADSHAPE / FPLX_E_NULL before any launch.
 *  wsl_gatedcrf_fwd: GatedCRFLoss.forward with the Potts shortcut and no masks.  desc: host fp32 [nk][3] = (weight, sigma_xy,
 *             sigma_rgb), 1 <= nk <= 4; a sigma of 0: that modality is absent (at least one per descriptor); 1 <= radius <= 8.
 *             For a pixel i of a slice and every window position j != i, |dy|, |dx| <= radius:
 *               k_ij = sum_desc weight exp(-1/2 (|xy_i - xy_j|^2 / sigma_xy^2 + sum_ch (I_i - I_j)^2 / sigma_rgb^2)).
 *             A j outside the slice still counts: the reference zero-pads its unfold, so such a j has xy = (0, 0), I = 0, p = 0.
 *             out0 = sum_i sum_j k_ij (1 - [j inside] sum_c p_c(i) p_c(j)) (one sum of non-negative terms), out3 = N D H W,
 *             out2 = loss = out0 / out3, out1 = 0.  kp fp32 [N][C][D][H][W]: kp_c(i) = sum_{j inside} k_ij p_c(j).
 *             part: fp32 [N D ceil(H / 16) ceil(W / 16)] (one per 16 x 16 tile of a slice; fewer than 2^31).
 *  wsl_gatedcrf_bwd: k is symmetric between pixels of the slice: e_c(i) = -2 kp_c(i) / out3.  The image takes no gradient.
 *  wsl_tv_fwd: TotalVariationLoss.forward for 5-D input: p' = 0.999 p + 5e-4 (a product, then a sum), e_v = min of p' over the
 *             in-bounds 3x3x3 window, o_v = max of e over the in-bounds window, contour_v = relu(o_v - e_v); out0 = sum contour,
 *             out3 = N C D H W, out2 = out0 / out3.  count int32 [N][C][D][H][W]: every voxel with contour_v > 0 adds +1 at the
 *             p' voxel whose value o_v is and -1 at the argmin of its own window; equal values take the first in (d, h, w) scan
 *             order, as torch's pooling does.  ws: at least 12 N C D H W bytes (p', e, the argmin offsets), 16-byte aligned
 *             (FPLX_E_BADSHAPE otherwise).
 *             part: fp32 [N C][fplx_loss_rows(D H W)].
 *  wsl_tv_bwd: e_c = 0.999 count_c / (N C D H W).
 *  wsl_mumford_shah_fwd: MumfordShahLoss.forward.  Per slice, class c, image channel ch: S0 = sum p_c, S1 = sum I_ch p_c over
 *             H x W, cen = S1 / S0 (no epsilon, as in the reference), level = sum (I_ch - cen)^2 p_c in a second pass.
 *             out0 = sum level; out1 = sum |p(h+1, w) - p(h, w)| + sum |p(h, w+1) - p(h, w)| inside the slice (penalty = 1) or
 *             their squares (penalty = 2); out3 = N C D H W; out2 = (out0 + lambda out1) / out3.  cen fp32 [N][D][Ci][C].
 *             part: fp32 [N D][fplx_loss_rows(H W)][C (1 + Ci)] (the moments; the loss pass reuses the front of it).
 *  wsl_mumford_shah_bwd: e_c(v) = (sum_ch (I_ch(v) - cen)^2 + lambda stencil_v) / out3 (the centroid's own derivative is 0:
 *             sum (I - cen) p = 0); stencil = sign(p_v - p_up) - sign(p_down - p_v) + the same along W, sign(0) = 0 (penalty 1),
 *             2 (p_v - p_up) - 2 (p_down - p_v) + the same along W (penalty 2); differences that leave the slice are absent. */
int fplx_wsl_gatedcrf_fwd(const float* logits, const float* image, int n, int c, int ci, int d, int h, int w, const float* desc,
                          int nk, int radius, int softmax, float* kp, float* part, double* out, fplx_stream_t stream);
int fplx_wsl_gatedcrf_bwd(const float* logits, const float* kp, const float* gscale, int n, int c, int d, int h, int w,
                          int softmax, float* dlogits, fplx_stream_t stream);
int fplx_wsl_tv_fwd(const float* logits, int n, int c, int d, int h, int w, int softmax, int32_t* count, void* ws,
                    size_t ws_bytes, float* part, double* out, fplx_stream_t stream);
int fplx_wsl_tv_bwd(const float* logits, const int32_t* count, const float* gscale, int n, int c, int d, int h, int w,
                    int softmax, float* dlogits, fplx_stream_t stream);
int fplx_wsl_mumford_shah_fwd(const float* logits, const float* image, int n, int c, int ci, int d, int h, int w, int penalty,
                              float lambda, int softmax, float* cen, float* part, double* out, fplx_stream_t stream);
int fplx_wsl_mumford_shah_bwd(const float* logits, const float* image, const float* cen, const float* gscale, int n, int c,
                              int ci, int d, int h, int w, int penalty, float lambda, int softmax, float* dlogits,
                              fplx_stream_t stream);

/* ------------------------------------------------------------------ noisy-label learning (csrc/nll.hip)
 * The selection losses of the reference's fourth entry point (PyMIC/pymic/net_run_nll/nll_co_teaching.py:91-118 CoTeaching,
 * nll_trinet.py:66-120 TriNet) over K = 1..3 networks.  Logits and the soft label fp32 [N][C][V] contiguous, 2 <= C <= 8,
 * 1 <= N <= 65535, N V < 2^31 (the bound of fplx_select_kth); a voxel has the flat index n V + v, the row order of the
 * reference's reshape_tensor_to_2D.  `logits`, `loss`, `mask`, `dlogits`: HOST arrays of K device pointers.  A lane takes four
 * voxels with 16-byte accesses where every base is 16-byte aligned and V is a multiple of 4, else one voxel.  Reductions: fp32
 * block partials summed in double in a fixed order by one wave, counts in integers - no floating-point atomics, two runs
 * give the same bits.  FPLX_E_NULL / FPLX_E_BADSHAPE / FPLX_E_WORKSPACE before any launch.
 *  nll_voxel_ce_fwd: ONE launch for all K, the label read once.  p = softmax(logits_k), p'_c = 0.999 p_c + 5e-4 (a product, then a
 *             sum, as torch's), loss_k[n V + v] = sum_c (-y_c) ln p'_c (c ascending).  part fp32 [K][N][fplx_nll_ce_rows(V)]: the
 *             block sums of loss_k, the partials of the reference's loss_no_select (nll_select_fwd adds them up).
 *  nll_select_mask: loss fp32 [n] -> mask uint8 [n] (1 = kept) from the order statistics fplx_select_kth wrote on the device.
 *             FPLX_NLL_RANK (CoTeaching, `ind_sorted[:num_remb]`): sk[0] = s[num_remb - 1] = t.  Kept: every voxel with
 *             loss < t and, of the voxels with loss == t, the first num_remb - #{loss < t} in index order - exactly num_remb
 *             voxels, the first num_remb entries of a STABLE ascending argsort.  Comparisons on select_kth's order-preserving
 *             integer key (all NaNs equal and last).  num_remb = n keeps all; num_remb = 0 keeps none (sk, ws may be NULL).
 *             Three passes - count, scan, write - in which every block owns the same contiguous chunk of the array; ws: at
 *             least fplx_nll_mask_ws_bytes().  w, smax are ignored.
 *             FPLX_NLL_BELOW (TriNet, `loss < torch.quantile(loss, q)`): sk = {s[k], s[k + 1]}, w in [0, 1) from the host:
 *             pos = float32(q) float32(n - 1) IN FP32 (torch makes q a tensor of the input's dtype), k = floor(pos),
 *             w = pos - k.  thr = torch's lerp in fp32: a + w (b - a) for w < 0.5, else b - (b - a)(1 - w), with b = a for
 *             w = 0 (torch gathers s[ceil(pos)]).  Kept iff loss < thr as fp32 values.  smax (optional): device s[n - 1]; if it
 *             is NaN the array holds a NaN, torch.quantile returns NaN and nothing is kept.  num_remb, ws are ignored.
 *  nll_select_fwd: ONE launch (after a memset node that clears its ticket).  loss_j fp32 [n], mask_j uint8 [n], uses[j]: bit i
 *             set = mask_i gates network j, the kept set of j is the AND of its masks (CoTeaching {2, 1}; TriNet {6, 5, 3}).
 *             out double [K][4]: sum of the kept loss_j; number kept; their quotient (0 / 0 = NaN, the mean of an empty
 *             selection as in the reference); sum of ALL loss_j from ce_part [K][ce_rows] (nll_voxel_ce_fwd's part,
 *             ce_rows = N fplx_nll_ce_rows(V)).  ws: at least fplx_nll_select_ws_bytes(); the block that draws the last ticket
 *             adds the rows up.
 *  nll_select_bwd: ONE launch for all K.  Softmax recomputed from the logits, count_j = out[j][1] read on the device:
 *             e_c = -0.999 y_c / p'_c keep_j / count_j, dlogits_j,c = gscale[0] wj p_c (e_c - sum_i p_i e_i); an empty
 *             selection gives zeros.  wj: 1 for CoTeaching (the sum of the two means), 1/3 for TriNet.  gscale: device fp32. */
enum { FPLX_NLL_RANK = 0, FPLX_NLL_BELOW = 1 };
int fplx_nll_ce_rows(int64_t voxels_per_sample);
int fplx_nll_voxel_ce_fwd(const float* const* logits, int k, const float* label, int n, int c, int64_t voxels_per_sample,
                          float* const* loss, float* part, fplx_stream_t stream);
size_t fplx_nll_mask_ws_bytes(void);
int fplx_nll_select_mask(const float* loss, int64_t n, int mode, int64_t num_remb, float w, const float* sk, const float* smax,
                         uint8_t* mask, void* ws, size_t ws_bytes, fplx_stream_t stream);
size_t fplx_nll_select_ws_bytes(void);
int fplx_nll_select_fwd(const float* const* loss, const uint8_t* const* mask, const int* uses, int k, int64_t n,
                        const float* ce_part, int64_t ce_rows, double* out, void* ws, size_t ws_bytes, fplx_stream_t stream);
int fplx_nll_select_bwd(const float* const* logits, const float* label, const uint8_t* const* mask, const int* uses, int k,
                        const double* out, const float* gscale, float wj, int n, int c, int64_t voxels_per_sample,
                        float* const* dlogits, fplx_stream_t stream);

/* ------------------------------------------------------------------ confident learning (csrc/cl.hip)
 * The producer of the mask SLSRLoss smooths with: what the reference's get_confident_map (PyMIC/pymic/net_run_nll/nll_clslsr.py:
 * 19-46) gets from cleanlab 1.0's get_noise_indices, as streaming passes.  psx fp32 PLANAR [C][M] (class plane c contiguous),
 * s uint8 [M] the given labels, 2 <= C <= 8, 1 <= M < 2^31 (the bound of fplx_select_kth).  A lane takes four voxels with 16-byte
 * accesses where the fp32 bases are 16-byte aligned, the byte arrays 4-byte aligned and M is a multiple of 4, else one voxel.
 * fp32 values are summed in double; block partials are added in a fixed order by one wave; counts are integers (integer
 * atomics) - no floating-point atomics, two runs give the same bits.  FPLX_E_NULL / FPLX_E_BADSHAPE / FPLX_E_WORKSPACE before
 * any launch.  A voxel with s >= C takes part in nothing but counts[C].
 *  cl_softmax: p[c][i] = softmax over c of x[.][i] in fp32: max, expf(x - max), the sum with c ascending, one division.  Written
 *             once; every later pass reads these stored bits, none recomputes them.
 *  cl_class_stats: counts int64 [C + 2]: counts[k] = #{s == k}, counts[C] = #{s >= C}, counts[C + 1] = #{voxels with a NaN in any
 *             plane}.  sums double [C]: sums[k] = sum over s_i == k of double(psx[k][i]).  thr double [C] (may be NULL) =
 *             sums[k] / counts[k], one division.  ws: at least fplx_cl_stats_ws_bytes(), 8-byte aligned; ONE launch after a memset
 *             node that clears its ticket.
 *  cl_confident_joint: conf_k = double(psx[k][i]) >= thr[k] - 1e-6 (float64).  No confident class: not counted; one: guess is that
 *             class; several: guess = the first maximum of psx[.][i] over ALL classes.  joint int64 [C][C]: joint[s_i][guess] += 1.
 *             joint is cleared by a memset node in front of the launch.
 *  cl_select_keys: j < 0: keys[i] = psx[k][i] where s_i == k, NaN elsewhere.  j >= 0 (j != k): keys[i] = -(psx[j][i] - psx[k][i])
 *             there (one fp32 rounding, the negation exact).  NaN sorts last in fplx_select_kth, so rank r of keys is rank r
 *             among the members for r < counts[k].
 *  cl_noise_mask: mask uint8 [M], count int64 [1] = the number of set voxels (cleared by a memset node).  With k = s_i:
 *             by_class = psx[k][i] < class_cut[k]; by_rate = some j with pair_active[k][j] and psx[j][i] - psx[k][i] >=
 *             pair_cut[k][j] (fp32, as the keys); mask = (by_class | by_rate | both of them, by `method`) and the first maximum
 *             of psx[.][i] != k.  class_cut fp32 [C] and pair_cut fp32 [C][C] are DEVICE arrays (the values fplx_select_kth wrote,
 *             pair_cut with the sign of the margin restored); pair_active uint8 [C][C] is a HOST array read before the call
 *             returns, its diagonal ignored.  A table the method does not use may be NULL.  Comparisons are on values, so
 *             voxels that tie at a cut are kept or dropped together. */
enum { FPLX_CL_BY_CLASS = 0, FPLX_CL_BY_NOISE_RATE = 1, FPLX_CL_BOTH = 2 };
int fplx_cl_softmax(const float* x, int c, int64_t m, float* p, fplx_stream_t stream);
size_t fplx_cl_stats_ws_bytes(void);
int fplx_cl_class_stats(const float* psx, const uint8_t* s, int c, int64_t m, void* ws, size_t ws_bytes, double* sums,
                        int64_t* counts, double* thr, fplx_stream_t stream);
int fplx_cl_confident_joint(const float* psx, const uint8_t* s, int c, int64_t m, const double* thr, int64_t* joint,
                            fplx_stream_t stream);
int fplx_cl_select_keys(const float* psx, const uint8_t* s, int c, int64_t m, int k, int j, float* keys, fplx_stream_t stream);
int fplx_cl_noise_mask(const float* psx, const uint8_t* s, int c, int64_t m, int method, const float* class_cut,
                       const float* pair_cut, const uint8_t* pair_active, uint8_t* mask, int64_t* count, fplx_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* FPLX_H */
